// Batched ray-cast renderer (mjl_render_qpos): RGB / depth / segmentation frames from qpos.
//
// Two launches per call:
//   render_setup_kernel   one wavefront per frame, lane = body: forward kinematics from qpos (the
//                         same BodyRec / JntRec records and level pass as `kinematics`), body
//                         inertial positions, the camera body's subtree centre of mass, and from
//                         them the frame's scene record: per geom the world centre, z axis, radius
//                         and half length, plus the camera pose and the checker plane's axes.
//   render_rays_kernel    grid = pixel tiles x frames, 256 threads = a 16 x 16 pixel tile, 8 x 8 per
//                         wavefront. The frame's scene record (1120 B) is copied to LDS once per
//                         block and read at block-uniform addresses (LDS broadcasts, no conflicts);
//                         one uniform loop over the geoms per ray with closed-form ray / plane,
//                         ray / sphere and ray / capsule tests, an optional second any-hit loop
//                         towards the light, shading (DESIGN.md "Rendering").
// The closed-form ray / plane, ray / sphere and ray / capsule tests are ray_scene.h's, shared with the ray casts
// (ray_kernels.hip).
// RGB is 3 bytes per pixel and a tile row starts at byte 3 (y W + x0), dword-aligned only for some
// widths; the tile's 768 bytes are staged in LDS and written with consecutive threads on
// consecutive bytes of a row (coalesced byte stores, the same code for every width, ragged tiles
// masked per byte).
// Included by capi.hip after step_kernels.hip (the model records, wave primitives and small math).
#pragma once

#include "ray_scene.h"

namespace mjl {

constexpr int kSceneGeom = 0;      // [MJL_MAXGEOM][8]: centre, radius (< 0: plane), z axis, half length (0: sphere)
constexpr int kSceneCamPos = 256;  // [3]
constexpr int kSceneCamMat = 260;  // [9] row-major, columns = the camera's x, y, z axes in the world
constexpr int kSceneChkX = 272;    // [3] the checker plane's x axis in the world
constexpr int kSceneChkY = 276;    // [3]
constexpr int kSceneFloats = 280;
constexpr float kShadowEps = 1e-3f;  // the shadow ray starts this far off the surface (metres)

struct RenderConst {  // per renderer, device global memory, read at uniform addresses
  int ngeom, checker_geom, light_directional, pad;
  float geom_rgb[MJL_MAXGEOM][4];
  float chk_rgb1[4], chk_rgb2[4];
  float chk_inv_cell[2], znear, zfar;
  float chk_x[4], chk_y[4];  // in the frame of the checker geom's body
  float sky1[4], sky2[4];
  float light_pos[4], light_dir[4], diffuse[4], ambient[4];
};
struct RenderCam {  // the selected camera, by value
  int body, mode;
  float tan_half;  // tan(fovy / 2)
  float pos[3], mat[9];
};

__global__ __launch_bounds__(64) void render_setup_kernel(const ModelF* __restrict__ mg, const RenderConst* __restrict__ rc,
                                                          RenderCam cam, const float* __restrict__ qpos,
                                                          float* __restrict__ scene) {
  MP m = uniform_ptr((MP)mg);
  const int lane = threadIdx.x, frame = blockIdx.x;
  const int nbody = m->nbody, ngeom = m->ngeom, maxlevel = m->maxlevel;
  const float* q = qpos + (size_t)frame * m->nq;
  float* S = scene + (size_t)frame * kSceneFloats;
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[isb ? lane : 0]);
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
  // tree pass: compose with the parent's world frame, one level at a time (frames stay in registers)
  float wp[3] = {0.f, 0.f, 0.f}, wq[4] = {1.f, 0.f, 0.f, 0.f};  // lane 0: the world frame
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
  // camera pose. fixed: the body's frame applied to the local pose; track / trackcom: the body's
  // position / subtree centre of mass plus the world offset of qpos0, rotation frozen at qpos0.
  const int cb = cam.body;
  float bmat[9];
  q2m(bmat, wq);
  float ip[3] = {0.f, 0.f, 0.f}, mass = 0.f;
  if (isb) {
    mv3(ip, bmat, br.ipos);
    ip[0] += wp[0]; ip[1] += wp[1]; ip[2] += wp[2];
    mass = br.mass;
  }
  const int cend = m->body_subtree_end[cb];
  const bool in = lane >= cb && lane < cend;
  const float ms = wsum(in ? mass : 0.f);
  const float c0 = wsum(in ? mass * ip[0] : 0.f), c1 = wsum(in ? mass * ip[1] : 0.f), c2 = wsum(in ? mass * ip[2] : 0.f);
  if (lane == cb) {
    float cp[3], cm[9];
    if (cam.mode == MJL_CAM_FIXED) {
      mv3(cp, bmat, cam.pos);
      cp[0] += wp[0]; cp[1] += wp[1]; cp[2] += wp[2];
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
          cm[3 * i + j] = bmat[3 * i] * cam.mat[j] + bmat[3 * i + 1] * cam.mat[3 + j] + bmat[3 * i + 2] * cam.mat[6 + j];
    } else {
      float base[3] = {wp[0], wp[1], wp[2]};
      if (cam.mode == MJL_CAM_TRACKCOM) {
        if (ms < kMinVal) { base[0] = ip[0]; base[1] = ip[1]; base[2] = ip[2]; }
        else { const float inv = 1.f / ms; base[0] = c0 * inv; base[1] = c1 * inv; base[2] = c2 * inv; }
      }
      for (int i = 0; i < 3; i++) cp[i] = base[i] + cam.pos[i];
      for (int i = 0; i < 9; i++) cm[i] = cam.mat[i];
    }
    for (int i = 0; i < 3; i++) S[kSceneCamPos + i] = cp[i];
    for (int i = 0; i < 9; i++) S[kSceneCamMat + i] = cm[i];
  }
  // geom frames: lane = geom, its body's frame from that body's lane
  const bool isg = lane < ngeom;
  const FrameRec fr = ldrec(&m->frec[isg ? lane : 0]);
  const int gb = isg ? fr.body : 0;
  float gq[4], gp[3];
#pragma unroll
  for (int i = 0; i < 3; i++) gp[i] = __shfl(wp[i], gb);
#pragma unroll
  for (int i = 0; i < 4; i++) gq[i] = __shfl(wq[i], gb);
  if (isg) {
    float gm[9], p[3], z[3];
    q2m(gm, gq);
    mv3(p, gm, fr.pos);
    mv3(z, gm, fr.mat);
    const int type = m->geom_type[lane];
    float* G = S + kSceneGeom + 8 * lane;
    G[0] = gp[0] + p[0]; G[1] = gp[1] + p[1]; G[2] = gp[2] + p[2];
    G[3] = type == MJL_GEOM_PLANE ? -1.f : m->geom_size[lane][0];
    G[4] = z[0]; G[5] = z[1]; G[6] = z[2];
    G[7] = type == MJL_GEOM_CAPSULE ? m->geom_size[lane][1] : 0.f;
    if (lane == rc->checker_geom) {
      float x[3], y[3];
      mv3(x, gm, rc->chk_x);
      mv3(y, gm, rc->chk_y);
      for (int i = 0; i < 3; i++) { S[kSceneChkX + i] = x[i]; S[kSceneChkY + i] = y[i]; }
    }
  }
}

__global__ __launch_bounds__(256) void render_rays_kernel(const RenderConst* __restrict__ rc, const float* __restrict__ scene,
                                                          float tan_half, int W, int H, int tiles_x, int shadows,
                                                          uint8_t* __restrict__ rgb, float* __restrict__ depth,
                                                          int* __restrict__ seg) {
  __shared__ f32x4 S4[kSceneFloats / 4];
  __shared__ uint8_t stage[16 * 48];
  const int t = threadIdx.x, frame = blockIdx.y;
  const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
  if (t < kSceneFloats / 4) S4[t] = ((const f32x4*)(scene + (size_t)frame * kSceneFloats))[t];
  __syncthreads();
  const float* S = (const float*)S4;
  // 8 x 8 pixels per wavefront, four wavefronts per 16 x 16 tile
  const int w = t >> 6, l = t & 63;
  const int lx = (w & 1) * 8 + (l & 7), ly = (w >> 1) * 8 + (l >> 3);
  const int px = tx * 16 + lx, py = ty * 16 + ly;
  const int ngeom = rc->ngeom;
  const float znear = rc->znear, zfar = rc->zfar;
  // the ray through the pixel centre: camera looks along -z, x right, y up
  const float u = (2.f * ((float)px + 0.5f) / (float)W - 1.f) * tan_half * ((float)W / (float)H);
  const float v = (1.f - 2.f * ((float)py + 0.5f) / (float)H) * tan_half;
  const float o[3] = {S[kSceneCamPos], S[kSceneCamPos + 1], S[kSceneCamPos + 2]};
  float d[3];
#pragma unroll
  for (int i = 0; i < 3; i++) d[i] = S[kSceneCamMat + 3 * i] * u + S[kSceneCamMat + 3 * i + 1] * v - S[kSceneCamMat + 3 * i + 2];
  {
    const float inv = 1.f / sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] *= inv; d[1] *= inv; d[2] *= inv;
  }
  float tbest = INFINITY;
  int hit = -1;
  for (int g = 0; g < ngeom; g++) {
    const float tg = ray_geom(S4[2 * g], S4[2 * g + 1], o, d, znear, zfar);
    if (tg < tbest) { tbest = tg; hit = g; }
  }
  float col[3];
  if (hit < 0) {
    const float s = 0.5f * (1.f + d[2]);
#pragma unroll
    for (int i = 0; i < 3; i++) col[i] = (1.f - s) * rc->sky2[i] + s * rc->sky1[i];
  }
  // surface point, normal, base colour, light direction (lanes without a hit carry dummies through
  // the shadow loop: the loop is uniform)
  float p[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 1.f}, Ld[3] = {0.f, 0.f, 1.f}, lam = 0.f, tl = INFINITY;
  if (hit >= 0) {
    const f32x4 A = S4[2 * hit], B = S4[2 * hit + 1];
#pragma unroll
    for (int i = 0; i < 3; i++) p[i] = o[i] + tbest * d[i];
    if (A.w < 0.f) {  // plane: the side facing the ray
      const float sg = (B.x * d[0] + B.y * d[1] + B.z * d[2]) < 0.f ? 1.f : -1.f;
      nrm[0] = sg * B.x; nrm[1] = sg * B.y; nrm[2] = sg * B.z;
    } else {  // sphere / capsule: away from the nearest point of the axis segment
      const float vv[3] = {p[0] - A.x, p[1] - A.y, p[2] - A.z};
      const float s = fminf(fmaxf(vv[0] * B.x + vv[1] * B.y + vv[2] * B.z, -B.w), B.w);
      const float ir = 1.f / A.w;
      nrm[0] = (vv[0] - s * B.x) * ir; nrm[1] = (vv[1] - s * B.y) * ir; nrm[2] = (vv[2] - s * B.z) * ir;
    }
    if (rc->light_directional) {
      Ld[0] = -rc->light_dir[0]; Ld[1] = -rc->light_dir[1]; Ld[2] = -rc->light_dir[2];
    } else {
      Ld[0] = rc->light_pos[0] - p[0]; Ld[1] = rc->light_pos[1] - p[1]; Ld[2] = rc->light_pos[2] - p[2];
      tl = sqrtf(Ld[0] * Ld[0] + Ld[1] * Ld[1] + Ld[2] * Ld[2]);
      const float inv = 1.f / tl;
      Ld[0] *= inv; Ld[1] *= inv; Ld[2] *= inv;
    }
    lam = fmaxf(0.f, nrm[0] * Ld[0] + nrm[1] * Ld[1] + nrm[2] * Ld[2]);
  }
  if (shadows && __syncthreads_or(lam > 0.f)) {  // hard shadow: any geom between the surface and the light
    const float so[3] = {p[0] + kShadowEps * nrm[0], p[1] + kShadowEps * nrm[1], p[2] + kShadowEps * nrm[2]};
    bool occ = false;
    for (int g = 0; g < ngeom; g++) occ = occ || ray_geom(S4[2 * g], S4[2 * g + 1], so, Ld, 0.f, tl) < INFINITY;
    if (occ) lam = 0.f;
  }
  if (hit >= 0) {
    float base[3] = {rc->geom_rgb[hit][0], rc->geom_rgb[hit][1], rc->geom_rgb[hit][2]};
    if (hit == rc->checker_geom) {
      const f32x4 A = S4[2 * hit];
      const float vv[3] = {p[0] - A.x, p[1] - A.y, p[2] - A.z};
      const float cu = vv[0] * S[kSceneChkX] + vv[1] * S[kSceneChkX + 1] + vv[2] * S[kSceneChkX + 2];
      const float cv = vv[0] * S[kSceneChkY] + vv[1] * S[kSceneChkY + 1] + vv[2] * S[kSceneChkY + 2];
      const int par = ((int)floorf(cu * rc->chk_inv_cell[0]) + (int)floorf(cv * rc->chk_inv_cell[1])) & 1;
#pragma unroll
      for (int i = 0; i < 3; i++) base[i] *= par ? rc->chk_rgb2[i] : rc->chk_rgb1[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) col[i] = base[i] * (rc->ambient[i] + rc->diffuse[i] * lam);
  }
  const bool inb = px < W && py < H;
  const size_t pix = ((size_t)frame * H + py) * W + px;
  if (inb && depth) depth[pix] = tbest;
  if (inb && seg) seg[pix] = hit;
  if (rgb) {
#pragma unroll
    for (int i = 0; i < 3; i++) stage[ly * 48 + lx * 3 + i] = (uint8_t)(fminf(fmaxf(col[i], 0.f), 1.f) * 255.f + 0.5f);
    __syncthreads();
    const int vw = min(16, W - tx * 16) * 3, vh = min(16, H - ty * 16);  // the tile's valid bytes per row, rows
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int e = t + 256 * k, row = e / 48, byte = e % 48;
      if (row < vh && byte < vw)
        rgb[(((size_t)frame * H + ty * 16 + row) * W + tx * 16) * 3 + byte] = stage[e];
    }
  }
}

}  // namespace mjl
