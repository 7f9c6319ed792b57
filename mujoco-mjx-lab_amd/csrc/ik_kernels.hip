// Batched inverse kinematics (mjl_ik): the damped least-squares iteration of include/mjx355.h, every iteration of
// one env's solve inside one launch. One wavefront per env; the iterate lives in LDS, the normal matrix in registers.
//
// A kernel of its own with a workspace of its own (8.1 KB of LDS); dyn_kernels.hip's helpers are called, not
// changed: dyn_tree_pass (the positions-only tree pass), dyn_dof_axis (the dof's world axis and anchor), and
// mass_matrix_kernel's factor and substitutions are repeated here on H.
//
// ik_kernel, per iteration k
//   1. dyn_tree_pass on the iterate (LDS).
//   2. lane = task: the world point, e_p, e_r into the residual stage es[t][6] (zeros where a row has no target
//      array), the lane's weighted residual norm; res = their maximum by readlane, in task order.
//   3. k = iterations, or tol > 0 and res < tol: out of the loop. res is the same in every lane and goes through
//      readfirstlane, so the loop's exit is a scalar branch.
//   4. lane = dof (both halves of the wave hold the same rows, d = lane & 31): the dof's axis and anchor into
//      registers, row d of H = (damping + posture) I and g_d = posture * delta_d. Then task by task: the six
//      weighted Jacobian entries c_r[d] of column d into the stage Js[6][32] (a dropped triple is skipped, a scalar
//      branch on the weights), a barrier, and a[j] = fma(c_r[d], Js[r][j], a[j]), g = fma(c_r[d], w e_r, g):
//      LDS does not grow with ntask.
//   5. The right-looking Cholesky factor on the rows in registers, L through the LDS stage into column registers,
//      the two substitutions by readlane; the step bound (a 32-step readlane maximum).
//   6. dq into LDS; lane = dof: a hinge or a free translation adds its entry (a limited hinge is clamped), the lane
//      of a free joint's first rotation dof advances the quaternion (unless its three entries of dq are zero).
// After the loop the residual stage holds e at the returned iterate: err is stored from it, qpos_out from the iterate.
//
// ik_kernel<true> (mjl_ik_wb) is the same iteration with a centre-of-mass task and one-sided clearance rows, each
// phase behind `if constexpr (WB)`, so ik_kernel<false> (mjl_ik) is the kernel above, instruction for instruction:
//   2a. (a CoM task) lane = body: xipos and the env's own mass into LDS; lane = subtree root: its mass and centre of
//       mass (cent_subtree_com, centroidal_dev.h). e_c = com_target - centre of mass of com_body, the same in every
//       lane; res takes com_weight[a] |e_c[a]|.
//   2b. (npair > 0) lane = geom: the scene record (scene_geom_record, ray_kernels.hip) and its body into LDS;
//       lane = pair: dist_pair (distance_dev.h), the pair's witness points, normal and bodies into the pair stage,
//       dist and the residual clear_min - dist in the lane's registers; a pair with dist < clear_min is active; res
//       takes clear_weight max(0, clear_min - dist) by readlane, in pair order.
//   4a. after the frame tasks, the CoM rows: column d of jac_com (cent_column) times com_weight into rows 0..2 of
//       the stage Js, then the same fma chain as a frame task's position rows, x, y, z.
//   4b. then the active pairs in index order (a scalar branch on the pair's weight, read by readlane): lane d's entry
//       of the gradient row (dist_jac_entry) times clear_weight into row 0 of Js, one more pass of the chain.
// After the loop com_err is stored from e_c and clearance from the pair lanes' dist. 3840 B more LDS, whatever npair.
// Included by capi.hip after dyn_kernels.hip.
#pragma once

#include <type_traits>

#include "centroidal_dev.h"
#include "distance_dev.h"
#include "ray_kernels.hip"

namespace mjl {

struct IkArgs {
  const ModelF* m;       // the shared model block (no geometric field is per-env)
  const DynTab* tab;
  const float* qstart;   // [nenv, nq]: the caller's start or the batch's qpos
  const float* qref;     // [nenv, nq] or null: the model's qpos0
  const float* mask;     // [nenv] or null
  int nenv, ntask;
  const int32_t* body;   // [ntask]
  const float* offset;   // [ntask, 3] or null
  const float* tpos;     // [nenv, ntask, 3] or null
  const float* tquat;    // [nenv, ntask, 4] or null
  const float* weight;   // [ntask, 2] or null
  uint32_t dofmask;
  int iterations, limits;
  float damping, posture, max_step, tol;
  float* qout;           // [nenv, nq]
  float* err;            // [nenv, ntask, 6] or null
  int32_t* niter;        // [nenv] or null
};

constexpr int kIkMaxTask = 32;
constexpr int kIkMaxPair = 32;

// mjl_ik_wb: IkArgs and the whole-body tasks. The small tables are host arrays copied into the kernel arguments.
struct IkWbArgs : IkArgs {
  const ModelF* m_env;    // [nenv] per-env blocks (the masses of the CoM task), or null
  const float* com_target;  // [nenv, 3] or null (no CoM task)
  int com_body;           // -1: no CoM task
  int npair;
  float com_weight[3];    // <= 0: the row is dropped
  uint8_t geom1[kIkMaxPair], geom2[kIkMaxPair];
  float clear_min[kIkMaxPair], clear_weight[kIkMaxPair];
  float* com_err;         // [nenv, 3] or null
  float* clearance;       // [nenv, npair] or null
};

// the rotation vector of the unit quaternion q (its scalar part made non-negative): mju_quat2Vel at dt = 1
static INL void ik_rotvec(float* r, const float* q) {
  const float sg = q[0] < 0.f ? -1.f : 1.f;
  const float v[3] = {sg * q[1], sg * q[2], sg * q[3]};
  const float n = sqrtf(dot3(v, v));
  const float s = n < kMinVal ? 0.f : 2.f * atan2f(n, sg * q[0]) / n;
  for (int i = 0; i < 3; i++) r[i] = v[i] * s;
}

template <bool WB>
__global__ __launch_bounds__(64) void ik_kernel(std::conditional_t<WB, IkWbArgs, IkArgs> A) {
  constexpr int NV = MJL_MAXV, LD = kDynLD;
  __shared__ float qpos[MJL_MAXQ], qref[MJL_MAXQ];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float dax[NV][3], danc[NV][3];
  __shared__ float xs[kIkMaxTask][3];    // the tasks' world points
  __shared__ float es[kIkMaxTask * 6];   // the residual stage: (e_p ; e_r) per task
  __shared__ __attribute__((aligned(16))) float Js[6][NV];  // one task's weighted Jacobian rows
  __shared__ float dqs[NV];
  __shared__ float Ms[NV * LD];          // L's rows in for its columns
  // The whole-body tasks' workspace. ik_kernel<false> declares one element of each and never names it (every use
  // stands in an `if constexpr (WB)` block), so the compiler drops them: mjl_ik's 8320 B of LDS rest on that
  // elimination. `make resource-usage` shows it; a use outside those blocks would grow mjl_ik's LDS.
  __shared__ float xim[WB ? MJL_MAXBODY : 1][4];  // xipos, mass
  __shared__ float cm[WB ? MJL_MAXBODY : 1][4];   // subtree: centre of mass, mass
  __shared__ int ssend[WB ? MJL_MAXBODY : 1];
  __shared__ f32x4 S4[WB ? 2 * MJL_MAXGEOM : 1];  // the geoms' scene records
  __shared__ int gbody[WB ? MJL_MAXGEOM : 1];
  __shared__ float P[WB ? kIkMaxPair * kDistStage : 1];  // the pairs' witness points, normals and bodies
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)A.m);
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel, ntask = A.ntask;
  const float nan = __int_as_float(0x7fc00000);

  // ---- a body id outside the model: NaN rows (uniform over the wave, and over the envs)
  bool anybad = false;
  for (int t = 0; t < ntask; t++) {
    const int b = A.body[t];
    anybad = anybad || b < 0 || b >= nbody;
  }
  if (anybad) {
    if (lane < nq) A.qout[(size_t)env * nq + lane] = nan;
    if (A.err)
      for (int i = lane; i < ntask * 6; i += 64) A.err[(size_t)env * ntask * 6 + i] = nan;
    if (A.niter && lane == 0) A.niter[env] = 0;
    if constexpr (WB) {
      if (A.com_err && lane < 3) A.com_err[(size_t)env * 3 + lane] = nan;
      if (A.clearance && lane < A.npair) A.clearance[(size_t)env * A.npair + lane] = nan;
    }
    return;
  }

  if (lane < nq) {
    qpos[lane] = A.qstart[(size_t)env * nq + lane];
    qref[lane] = A.qref ? A.qref[(size_t)env * nq + lane] : m->qpos0[lane];
  }
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    xpos[0][0] = xpos[0][1] = xpos[0][2] = 0.f;
  }
  if (lane < NV)
    for (int i = 0; i < 3; i++) dax[lane][i] = danc[lane][i] = 0.f;
  __syncthreads();
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);

  // ---- lane = task: the task's constants
  const bool ist = lane < ntask;
  const int tb = ist ? A.body[lane] : 0;
  float toff[3] = {0.f, 0.f, 0.f}, tp[3] = {0.f, 0.f, 0.f}, tq[4] = {1.f, 0.f, 0.f, 0.f};
  float twp = 0.f, twr = 0.f;
  if (ist) {
    if (A.offset)
      for (int i = 0; i < 3; i++) toff[i] = A.offset[lane * 3 + i];
    if (A.tpos)
      for (int i = 0; i < 3; i++) tp[i] = A.tpos[((size_t)env * ntask + lane) * 3 + i];
    if (A.tquat) {
      for (int i = 0; i < 4; i++) tq[i] = A.tquat[((size_t)env * ntask + lane) * 4 + i];
      qnorm(tq);
    }
    const float wp = A.weight ? A.weight[lane * 2] : 1.f, wr = A.weight ? A.weight[lane * 2 + 1] : 1.f;
    twp = (A.tpos && wp > 0.f) ? wp : 0.f;
    twr = (A.tquat && wr > 0.f) ? wr : 0.f;
  }

  // ---- lane = dof in both halves of the wave: the dof's record, its qpos address, whether it may move
  const int d = lane & 31;
  const bool isd = d < nv;
  const DofRec dr = ldrec(&m->drec[isd ? d : 0]);
  const JntRec dj = ldrec(&m->jrec[max(0, min(dr.jntid, MJL_MAXJNT - 1))]);
  const int kf = dr.kfree;
  const bool active = isd && ((A.dofmask >> d) & 1u);
  const int qa = kf < 0 ? dj.qadr : (kf < 3 ? dj.qadr + kf : dj.qadr + 3);  // a rotation dof: the quaternion
  float lim_lo = 0.f, lim_hi = 0.f;
  bool limited = false;
  if (A.limits && isd && kf < 0) {
    const LimRec lr = ldrec(&m->jlim[max(0, min(dr.jntid, MJL_MAXJNT - 1))]);
    limited = lr.on != 0;
    lim_lo = lr.lo; lim_hi = lr.hi;
  }
  const float diag0 = A.damping + A.posture;

  // ---- the whole-body tasks' constants (WB): lane = body its own mass, lane = pair the pair's record
  [[maybe_unused]] bool hascom = false, ispair = false;
  [[maybe_unused]] float bmass = 0.f, bipos[3] = {0.f, 0.f, 0.f}, cw[3] = {0.f, 0.f, 0.f}, ct[3] = {0.f, 0.f, 0.f};
  [[maybe_unused]] float ec[3] = {0.f, 0.f, 0.f}, pcmin = 0.f, pcw = 0.f, pdist = 0.f, pres = 0.f, pwact = 0.f;
  [[maybe_unused]] int pg1 = 0, pg2 = 0, send = 0, db = 0, ngeom = 0;
  if constexpr (WB) {
    hascom = A.com_body >= 0 && A.com_body < nbody;
    if (hascom) {
      const MP me = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));  // the env's own masses
      if (lane > 0 && lane < nbody) {
        bmass = me->brec[lane].mass;
        for (int i = 0; i < 3; i++) bipos[i] = me->brec[lane].ipos[i];
      }
      for (int i = 0; i < 3; i++) {
        cw[i] = A.com_weight[i] > 0.f ? A.com_weight[i] : 0.f;
        ct[i] = A.com_target[(size_t)env * 3 + i];
      }
      send = lane < nbody ? max(lane + 1, min(br.subtree_end, nbody)) : 0;
      db = max(0, min(dr.bodyid, nbody - 1));
    }
    ngeom = min(m->ngeom, MJL_MAXGEOM);
    ispair = lane < A.npair;
    if (ispair) {
      pg1 = min((int)A.geom1[lane], ngeom - 1);
      pg2 = min((int)A.geom2[lane], ngeom - 1);
      pcmin = A.clear_min[lane];
      pcw = A.clear_weight[lane] > 0.f ? A.clear_weight[lane] : 0.f;
    }
  }

  int k = 0;
  for (;; k++) {
    dyn_tree_pass(m, br, qpos, xpos, xquat, dax, danc, nbody, maxlevel, lane);

    // ---- lane = task: the point and the residuals
    float resl = 0.f;
    if (ist) {
      float R[9], x[3], e[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      q2m(R, xquat[tb]);
      mv3(x, R, toff);
      for (int i = 0; i < 3; i++) x[i] += xpos[tb][i];
      if (A.tpos) {
        for (int i = 0; i < 3; i++) e[i] = tp[i] - x[i];
        resl = twp * sqrtf(dot3(e, e));
      }
      if (A.tquat) {
        const float qc[4] = {xquat[tb][0], -xquat[tb][1], -xquat[tb][2], -xquat[tb][3]};
        float qe[4];
        qmul(qe, tq, qc);
        ik_rotvec(e + 3, qe);
        resl = fmaxf(resl, twr * sqrtf(dot3(e + 3, e + 3)));
      }
      for (int i = 0; i < 3; i++) xs[lane][i] = x[i];
      for (int i = 0; i < 6; i++) es[lane * 6 + i] = e[i];
    }
    float res = 0.f;
    for (int t = 0; t < ntask; t++) res = fmaxf(res, rdlane(resl, t));
    if constexpr (WB) {
      if (hascom) {  // ---- lane = body: xipos, mass; lane = subtree root: its mass and centre of mass
        float xi[3] = {0.f, 0.f, 0.f};
        if (lane > 0 && lane < nbody) {
          float R[9], dd[3];
          q2m(R, xquat[lane]);
          mv3(dd, R, bipos);
          for (int i = 0; i < 3; i++) xi[i] = xpos[lane][i] + dd[i];
        }
        if (lane < nbody) {
          for (int i = 0; i < 3; i++) xim[lane][i] = xi[i];
          xim[lane][3] = bmass;
          ssend[lane] = send;
        }
        __syncthreads();
        if (lane < nbody) {
          float ms, inv, c[3];
          bool empty;
          cent_subtree_com(xim, lane, send, xi, c, ms, inv, empty);
          for (int i = 0; i < 3; i++) cm[lane][i] = c[i];
          cm[lane][3] = empty ? 0.f : ms;
        }
        __syncthreads();
        for (int i = 0; i < 3; i++) {
          ec[i] = cw[i] > 0.f ? ct[i] - cm[A.com_body][i] : 0.f;
          res = fmaxf(res, cw[i] * fabsf(ec[i]));
        }
      }
      if (A.npair > 0) {  // ---- lane = geom: the scene record and the body; lane = pair: the distance
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
        if (ispair) {
          float from[3], to[3], n[3];
          pdist = dist_pair(S4[2 * pg1], S4[2 * pg1 + 1], S4[2 * pg2], S4[2 * pg2 + 1], from, to, n);
          const bool on = pdist < pcmin;
          pres = on ? pcmin - pdist : 0.f;
          pwact = on ? pcw : 0.f;
          float* s = P + lane * kDistStage;
          for (int i = 0; i < 3; i++) { s[i] = from[i]; s[3 + i] = to[i]; s[6 + i] = n[i]; }
          s[9] = __int_as_float(gbody[pg1]);
          s[10] = __int_as_float(gbody[pg2]);
          s[11] = 1.f;
        }
        for (int p = 0; p < A.npair; p++) res = fmaxf(res, rdlane(pwact, p) * rdlane(pres, p));
      }
    }
    __syncthreads();
    const bool stop = k >= A.iterations || (A.tol > 0.f && res < A.tol);
    if (__builtin_amdgcn_readfirstlane((int)stop)) break;

    // ---- lane = dof: the axis, row d of H and g_d
    float ax[3], an[3];
    const int kind = dyn_dof_axis(dr, isd ? d : 0, xpos, xquat, dax, danc, nbody, ax, an);
    float g = 0.f;
    if (A.posture > 0.f && active) {
      float del;
      if (kf < 3) {
        del = qref[qa] - qpos[qa];
      } else {
        float q0[4] = {qpos[qa], -qpos[qa + 1], -qpos[qa + 2], -qpos[qa + 3]};
        float q1[4] = {qref[qa], qref[qa + 1], qref[qa + 2], qref[qa + 3]};
        qnorm(q0);
        qnorm(q1);
        float qd[4], rv[3];
        qmul(qd, q0, q1);
        ik_rotvec(rv, qd);
        del = kf == 3 ? rv[0] : (kf == 4 ? rv[1] : rv[2]);
      }
      g = A.posture * del;
    }
    float a[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) a[j] = j == d ? (active ? diag0 : 1.f) : 0.f;

    for (int t = 0; t < ntask; t++) {
      const float wp = rdlane(twp, t), wr = rdlane(twr, t);
      if (!(wp > 0.f) && !(wr > 0.f)) continue;
      const int b = A.body[t];
      const bool moves = active && ((A.tab->body_dofmask[b] >> d) & 1u);
      float jr[3] = {0.f, 0.f, 0.f}, jp[3] = {0.f, 0.f, 0.f};
      if (moves) {
        if (kind == 1) {
          for (int i = 0; i < 3; i++) jp[i] = ax[i];
        } else {
          const float r[3] = {xs[t][0] - an[0], xs[t][1] - an[1], xs[t][2] - an[2]};
          for (int i = 0; i < 3; i++) jr[i] = ax[i];
          add_cross(jp, ax, r);
        }
      }
      float c[6];
      for (int i = 0; i < 3; i++) { c[i] = wp * jp[i]; c[3 + i] = wr * jr[i]; }
      if (lane < NV)
        for (int i = 0; i < 6; i++) Js[i][lane] = c[i];
      __syncthreads();
      if (wp > 0.f) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
          for (int j = 0; j < NV; j++) a[j] = fmaf(c[r], Js[r][j], a[j]);
          g = fmaf(c[r], wp * es[t * 6 + r], g);
        }
      }
      if (wr > 0.f) {
#pragma unroll
        for (int r = 3; r < 6; r++) {
#pragma unroll
          for (int j = 0; j < NV; j++) a[j] = fmaf(c[r], Js[r][j], a[j]);
          g = fmaf(c[r], wr * es[t * 6 + r], g);
        }
      }
      __syncthreads();
    }

    if constexpr (WB) {
      if (hascom) {  // ---- the CoM rows x, y, z: column d of jac_com, weighted
        const int S = cent_moved_set(A.tab, A.com_body, d, db, ssend, active);
        float jc[3], c[3];
        cent_column<false>(S, A.com_body, cm, nullptr, kind, ax, an, jc, nullptr);
        for (int i = 0; i < 3; i++) c[i] = cw[i] * jc[i];
        if (lane < NV)
          for (int i = 0; i < 3; i++) Js[i][lane] = c[i];
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < 3; r++) {
          if (!(cw[r] > 0.f)) continue;
          const float cr = r == 0 ? c[0] : (r == 1 ? c[1] : c[2]);
#pragma unroll
          for (int j = 0; j < NV; j++) a[j] = fmaf(cr, Js[r][j], a[j]);
          g = fmaf(cr, cw[r] * ec[r], g);
        }
        __syncthreads();
      }
#pragma unroll 1
      for (int p = 0; p < A.npair; p++) {  // ---- the active pairs: +w jac, residual w (clear_min - dist)
        const float w = rdlane(pwact, p), e = rdlane(pres, p);
        if (!(w > 0.f)) continue;
        const float c = active ? w * dist_jac_entry(A.tab, P + p * kDistStage, d, kind, ax, an) : 0.f;
        if (lane < NV) Js[0][lane] = c;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NV; j++) a[j] = fmaf(c, Js[0][j], a[j]);
        g = fmaf(c, w * e, g);
        __syncthreads();
      }
    }

    // ---- H = L L' (mass_matrix_kernel's factor), the columns of L through the stage, H dq = g
    float invd = 1.f;
#pragma unroll
    for (int kk = 0; kk < NV; kk++) {
      const float piv = rdlane(a[kk], kk);
      const float lkk = sqrtf(piv), inv = 1.f / lkk;
      a[kk] = (d == kk) ? lkk : a[kk] * inv;
      invd = (d == kk) ? inv : invd;
#pragma unroll
      for (int j = kk + 1; j < NV; j++) a[j] = fmaf(-a[kk], rdlane(a[kk], j), a[j]);
    }
    float cl[NV];
    if (lane < NV) {
#pragma unroll
      for (int j = 0; j < NV; j++) Ms[lane * LD + j] = a[j];
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < NV; kk++) cl[kk] = Ms[kk * LD + d];
    float x = g;
#pragma unroll
    for (int kk = 0; kk < NV; kk++) {  // L y = g
      const float yk = rdlane(x, kk) * rdlane(invd, kk);
      x = (d == kk) ? yk : (d > kk ? fmaf(-a[kk], yk, x) : x);
    }
#pragma unroll
    for (int kk = NV - 1; kk >= 0; kk--) {  // L' dq = y
      const float zk = rdlane(x, kk) * rdlane(invd, kk);
      x = (d == kk) ? zk : (d < kk ? fmaf(-cl[kk], zk, x) : x);
    }
    if (A.max_step > 0.f) {
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < NV; j++) s = fmaxf(s, fabsf(rdlane(x, j)));
      if (s > A.max_step) x *= A.max_step / s;
    }

    // ---- q <- integratePos(q, dq, 1) over the dofs that may move
    if (lane < NV) dqs[lane] = x;
    __syncthreads();
    if (lane < NV && active && kf < 3) {
      float v = qpos[qa] + x;
      if (limited) v = fminf(fmaxf(v, lim_lo), lim_hi);
      qpos[qa] = v;
    }
    if (lane < NV && isd && kf == 3) {
      float w[3] = {dqs[d], dqs[d + 1], dqs[d + 2]};
      const float nrm = norm3(w);
      float sn, cs;
      sincosf(0.5f * nrm, &sn, &cs);
      const float qr[4] = {cs, w[0] * sn, w[1] * sn, w[2] * sn};
      float qq[4] = {qpos[qa], qpos[qa + 1], qpos[qa + 2], qpos[qa + 3]};
      qmul(qq, qq, qr);
      qnorm(qq);
      if (nrm > 0.f)  // a zero step (its dofs outside dofmask, or no task moved by them) leaves the entries alone
        for (int i = 0; i < 4; i++) qpos[qa + i] = qq[i];
    }
    __syncthreads();
  }

  if (lane < nq) A.qout[(size_t)env * nq + lane] = qpos[lane];
  if (A.err)
    for (int i = lane; i < ntask * 6; i += 64) A.err[(size_t)env * ntask * 6 + i] = es[i];
  if (A.niter && lane == 0) A.niter[env] = k;
  if constexpr (WB) {
    if (A.com_err && lane < 3) A.com_err[(size_t)env * 3 + lane] = lane == 0 ? ec[0] : (lane == 1 ? ec[1] : ec[2]);
    if (A.clearance && ispair) A.clearance[(size_t)env * A.npair + lane] = pdist;
  }
}

}  // namespace mjl
