// Batched ray casts against the batch's current state (mjl_ray, mjl_ray_scan): mjx.ray / mj_ray, and ray
// patterns carried by a body or site frame (height scanner, lidar fan, rangefinder).
//
// One launch, one 64-lane wavefront per (env, chunk of `chunk` rays):
//   1. lane = body: forward kinematics from the env's qpos (scene_body_frames, as render_setup_kernel does
//      it), frames in registers. The stored xpos / xquat are neither read nor written.
//   2. lane = geom: the geom's scene record (centre, radius, z axis, half length: 32 B) into LDS, at most
//      MJL_MAXGEOM = 32 of them (1 KB). With a scan, the lane of the carrying body also writes the frame's
//      rotation and origin (12 floats) to LDS.
//   3. lanes stride over the chunk's rays; each ray loops over the geoms that pass the body filter (a bit mask
//      of geoms, uniform: a scalar test per geom), reading the records at wave-uniform LDS addresses
//      (broadcasts, no bank conflicts), with the renderer's closed-form tests (ray_scene.h).
// chunk >= nray is "kinematics once per env"; a smaller chunk repeats steps 1 and 2 in every chunk's wavefront
// and gives the device more of them. The host picks the chunk (kRayChunk, capi.hip; DESIGN.md "Rays" has the
// measurement).
// Included by capi.hip after step_kernels.hip and render_kernels.hip (ray_scene.h).
#pragma once

#include "ray_scene.h"

namespace mjl {

// Forward kinematics of one env on one wavefront, lane = body (render_setup_kernel's, restated here so that
// the renderer's kernel keeps its code to the instruction): the world frame of the lane's body into wp / wq
// (lane 0 and lanes past nbody: the world frame). `br` is the lane's body record (body 0's for a lane that is no body). Frames stay in
// registers; every lane of the wavefront must call (the level pass shuffles).
INL void scene_body_frames(MP m, const float* q, bool isb, const BodyRec& br, float* wp, float* wq) {
  const int maxlevel = m->maxlevel;
  // body transform relative to its parent (free joint: the world pose)
  float lp[3] = {0.f, 0.f, 0.f}, lq[4] = {1.f, 0.f, 0.f, 0.f};
  if (isb) {
    if (br.isfree) {
      const int qa = br.qadr;
      lp[0] = q[qa]; lp[1] = q[qa + 1]; lp[2] = q[qa + 2];
      lq[0] = q[qa + 3]; lq[1] = q[qa + 4]; lq[2] = q[qa + 5]; lq[3] = q[qa + 6];
      qnorm(lq);
    } else {
      lp[0] = br.pos[0]; lp[1] = br.pos[1]; lp[2] = br.pos[2];
      lq[0] = br.quat[0]; lq[1] = br.quat[1]; lq[2] = br.quat[2]; lq[3] = br.quat[3];
      for (int j = br.jntadr; j < br.jntadr + br.jntnum; j++) {  // hinges rotate about their anchor
        const JntRec jr = ldrec(&m->jrec[j]);
        float mat[9], anc[3], off[3], s, c;
        q2m(mat, lq);
        mv3(anc, mat, jr.pos);
        anc[0] += lp[0]; anc[1] += lp[1]; anc[2] += lp[2];
        sincosf(0.5f * (q[jr.qadr] - jr.qpos0), &s, &c);
        const float ql[4] = {c, jr.axis[0] * s, jr.axis[1] * s, jr.axis[2] * s};
        qmul(lq, lq, ql);
        q2m(mat, lq);
        mv3(off, mat, jr.pos);
        lp[0] = anc[0] - off[0]; lp[1] = anc[1] - off[1]; lp[2] = anc[2] - off[2];
      }
    }
  }
  // tree pass: compose with the parent's world frame, one level at a time
  wp[0] = wp[1] = wp[2] = 0.f;
  wq[0] = 1.f; wq[1] = wq[2] = wq[3] = 0.f;  // lane 0: the world frame
  const int par = isb ? br.parent : 0;
  for (int L = 1; L <= maxlevel; L++) {
    float pp[3], pq[4];
#pragma unroll
    for (int i = 0; i < 3; i++) pp[i] = __shfl(wp[i], par);
#pragma unroll
    for (int i = 0; i < 4; i++) pq[i] = __shfl(wq[i], par);
    if (isb && br.level == L) {
      if (br.isfree) {
        wp[0] = lp[0]; wp[1] = lp[1]; wp[2] = lp[2];
        wq[0] = lq[0]; wq[1] = lq[1]; wq[2] = lq[2]; wq[3] = lq[3];
      } else {
        float pm[9];
        q2m(pm, pq);
        mv3(wp, pm, lp);
        wp[0] += pp[0]; wp[1] += pp[1]; wp[2] += pp[2];
        qmul(wq, pq, lq);
        qnorm(wq);
      }
    }
  }
}

// The scene record of geom g (frame constants fr) on a body with world rotation gm and origin gp:
// G[0..2] centre, G[3] radius (< 0: plane), G[4..6] z axis, G[7] half length (0: sphere).
INL void scene_geom_record(MP m, int g, const FrameRec& fr, const float* gm, const float* gp, float* G) {
  float p[3], z[3];
  mv3(p, gm, fr.pos);
  mv3(z, gm, fr.mat);
  const int type = m->geom_type[g];
  G[0] = gp[0] + p[0]; G[1] = gp[1] + p[1]; G[2] = gp[2] + p[2];
  G[3] = type == MJL_GEOM_PLANE ? -1.f : m->geom_size[g][0];
  G[4] = z[0]; G[5] = z[1]; G[6] = z[2];
  G[7] = type == MJL_GEOM_CAPSULE ? m->geom_size[g][1] : 0.f;
}

struct RayArgs {
  const ModelF* m;
  const float* qpos;   // [nenv, nq]
  const float* mask;   // [nenv] or null
  const float* pnt;    // world rays: [nenv, nray, 3]; scan: [nray, 3] in the frame
  const float* vec;
  int nenv, nray, chunk, nchunk;
  int scan;            // 0: world rays (mjl_ray); 1: rays of a frame (mjl_ray_scan)
  int objtype, objid, align;
  int flags, bodyexclude;
  float cutoff;
  float* dist;         // [nenv, nray]
  int* geomid;         // [nenv, nray] or null
  float* hitpos;       // [nenv, nray, 3] or null
};

__global__ __launch_bounds__(64) void rays_kernel(RayArgs A) {
  __shared__ f32x4 S4[2 * MJL_MAXGEOM];
  __shared__ float F[12];  // scan: the frame's rotation (row-major) and origin
  MP m = uniform_ptr((MP)A.m);
  const int lane = threadIdx.x;
  const int env = blockIdx.x / A.nchunk, c = blockIdx.x % A.nchunk;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const int nbody = m->nbody, ngeom = min(m->ngeom, MJL_MAXGEOM);
  const float* q = A.qpos + (size_t)env * m->nq;
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[isb ? lane : 0]);
  float wp[3], wq[4];
  scene_body_frames(m, q, isb, br, wp, wq);

  if (A.scan) {  // the frame: an xbody's, or a site's on its body (as the pos-stage sensors define them)
    int fb = A.objid;
    float fpos[3] = {0.f, 0.f, 0.f}, fmat[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (A.objtype == MJL_OBJ_SITE) {
      const FrameRec sr = ldrec(&m->frec[kSiteLane + A.objid]);
      fb = sr.body;
#pragma unroll
      for (int i = 0; i < 3; i++) fpos[i] = sr.pos[i];
#pragma unroll
      for (int i = 0; i < 9; i++) fmat[i] = sr.mat[i];
    }
    if (lane == fb) {
      float bm[9], d[3], R[9];
      q2m(bm, wq);
      mv3(d, bm, fpos);
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
          R[3 * i + j] = bm[3 * i] * fmat[j] + bm[3 * i + 1] * fmat[3 + j] + bm[3 * i + 2] * fmat[6 + j];
      if (A.align == MJL_SCAN_YAW) {  // the rotation about world z by the frame's heading
        const float x = R[0], y = R[3], n2 = x * x + y * y;
        float cs = 1.f, sn = 0.f;
        if (!(n2 < 1e-12f)) { const float inv = 1.f / sqrtf(n2); cs = x * inv; sn = y * inv; }
        R[0] = cs; R[1] = -sn; R[2] = 0.f;
        R[3] = sn; R[4] = cs; R[5] = 0.f;
        R[6] = 0.f; R[7] = 0.f; R[8] = 1.f;
      }
#pragma unroll
      for (int i = 0; i < 9; i++) F[i] = R[i];
#pragma unroll
      for (int i = 0; i < 3; i++) F[9 + i] = wp[i] + d[i];
    }
  }

  // geom records: lane = geom, its body's frame from that body's lane
  const bool isg = lane < ngeom;
  const FrameRec fr = ldrec(&m->frec[isg ? lane : 0]);
  const int gb = isg ? fr.body : 0;
  float gq[4], gp[3];
#pragma unroll
  for (int i = 0; i < 3; i++) gp[i] = __shfl(wp[i], gb);
#pragma unroll
  for (int i = 0; i < 4; i++) gq[i] = __shfl(wq[i], gb);
  if (isg) {
    float gm[9], rec[8];
    q2m(gm, gq);
    scene_geom_record(m, lane, fr, gm, gp, rec);
    S4[2 * lane] = f32x4{rec[0], rec[1], rec[2], rec[3]};
    S4[2 * lane + 1] = f32x4{rec[4], rec[5], rec[6], rec[7]};
  }
  __syncthreads();

  // the body filter as a mask of geoms (uniform)
  uint32_t allow = ngeom >= 32 ? 0xffffffffu : ((1u << ngeom) - 1u);
  if (!(A.flags & MJL_RAY_STATIC)) allow &= ~m->body_geommask[0];
  if (A.bodyexclude >= 0) allow &= ~m->body_geommask[A.bodyexclude];
  allow = __builtin_amdgcn_readfirstlane(allow);

  const int r1 = min(A.nray, (c + 1) * A.chunk);
  for (int r = c * A.chunk + lane; r < r1; r += 64) {
    float o[3], v[3];
    if (A.scan) {
      const float lo[3] = {A.pnt[3 * r], A.pnt[3 * r + 1], A.pnt[3 * r + 2]};
      const float lv[3] = {A.vec[3 * r], A.vec[3 * r + 1], A.vec[3 * r + 2]};
      mv3(o, F, lo);
      mv3(v, F, lv);
      o[0] += F[9]; o[1] += F[10]; o[2] += F[11];
    } else {
      const size_t k = 3 * ((size_t)env * A.nray + r);
#pragma unroll
      for (int i = 0; i < 3; i++) { o[i] = A.pnt[k + i]; v[i] = A.vec[k + i]; }
    }
    // the tests take a unit direction: t is found along vec / |vec| and scaled back (a zero vec misses)
    const float len = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const float inv = 1.f / len;
    const float d[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    const float tmax = A.cutoff > 0.f ? A.cutoff * len : INFINITY;
    float tbest = INFINITY;
    int hit = -1;
    if (len > 0.f && len < INFINITY) {
      for (int g = 0; g < ngeom; g++) {
        if (!((allow >> g) & 1u)) continue;
        const float tg = ray_geom(S4[2 * g], S4[2 * g + 1], o, d, 0.f, tmax);
        if (tg < tbest) { tbest = tg; hit = g; }
      }
    }
    const float t = hit >= 0 ? tbest * inv : -1.f;
    const size_t e = (size_t)env * A.nray + r;
    A.dist[e] = t;
    if (A.geomid) A.geomid[e] = hit;
    if (A.hitpos) {
      const float s = hit >= 0 ? t : 0.f;
#pragma unroll
      for (int i = 0; i < 3; i++) A.hitpos[3 * e + i] = o[i] + s * v[i];
    }
  }
}

}  // namespace mjl
