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
// Included by capi.hip after dyn_kernels.hip.
#pragma once

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

// the rotation vector of the unit quaternion q (its scalar part made non-negative): mju_quat2Vel at dt = 1
static INL void ik_rotvec(float* r, const float* q) {
  const float sg = q[0] < 0.f ? -1.f : 1.f;
  const float v[3] = {sg * q[1], sg * q[2], sg * q[3]};
  const float n = sqrtf(dot3(v, v));
  const float s = n < kMinVal ? 0.f : 2.f * atan2f(n, sg * q[0]) / n;
  for (int i = 0; i < 3; i++) r[i] = v[i] * s;
}

__global__ __launch_bounds__(64) void ik_kernel(IkArgs A) {
  constexpr int NV = MJL_MAXV, LD = kDynLD;
  __shared__ float qpos[MJL_MAXQ], qref[MJL_MAXQ];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float dax[NV][3], danc[NV][3];
  __shared__ float xs[kIkMaxTask][3];    // the tasks' world points
  __shared__ float es[kIkMaxTask * 6];   // the residual stage: (e_p ; e_r) per task
  __shared__ __attribute__((aligned(16))) float Js[6][NV];  // one task's weighted Jacobian rows
  __shared__ float dqs[NV];
  __shared__ float Ms[NV * LD];          // L's rows in for its columns
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
}

}  // namespace mjl
