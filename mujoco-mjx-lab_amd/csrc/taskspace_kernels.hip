// Task-space dynamics readout (mjl_jac_dot, mjl_centroidal): the time derivatives of mjl_jac's point Jacobians
// and the velocity-product term Jdot qvel, the Jacobian of a subtree's centre of mass, the angular-momentum
// matrix about it and their bias, as include/mjx355.h defines them.
//
// Two kernels of their own, each with a workspace of its own (LDS): nothing of the step kernel's workspace or
// phases is touched, and jac_kernel / mass_matrix_kernel and their helpers (dyn_kernels.hip) are used as they
// are, not changed. One wavefront per env. Both start with ts_tree_pass: dyn_tree_pass's frames, axes and anchors
// together with the rates of body_data_kernel's pass at qacc = 0 (w, the origin's v and, for the centroidal
// bias, dw/dt and a), and per hinge dof the angular velocity and the anchor velocity of the frame that carries
// the axis: the rates of the chain before the hinge itself, read off while the body's hinges are peeled.
//
// jac_dot_kernel
//   1. qpos, qvel into LDS; the tree pass; lane = dof (both halves of the wave, d = lane & 31): axis a and anchor
//      p as jac_kernel, and their rates: a hinge's da/dt = w_pre x a, dp/dt = v_pre(p) out of LDS; a free
//      rotation's da/dt = w_b x a, dp/dt = the free joint's linear rates; a free translation's are zero.
//   2. Points two at a time as jac_kernel: x, dx/dt = v_b + w_b x (x - xpos_b), the body's dof mask, column d of
//      jacr_dot (da/dt) and jacp_dot (da/dt x (x - p) + a x (dx/dt - dp/dt)) into one LDS stage per output, then
//      dyn_emit's coalesced stores. jdotv: the six column-times-qvel products summed over the 32 lanes of the
//      half by a butterfly (one fixed order): the matrix product itself, so it agrees with jacp_dot qvel to the
//      rounding of a 32-term sum; with jdotv alone nothing nv-wide is staged or stored.
// centroidal_kernel (env e on its own model block while per-env model parameters are on)
//   1. qpos, qvel into LDS; the tree pass with accelerations.
//   2. lane = body: xipos, the world inertia, the centre of mass's velocity-product acceleration, the body's own
//      momentum rates [m a ; I dw + w x I w]; lane = subtree root s: mass, centre of mass, the inertia about that
//      centre (one loop over the contiguous subtree out of LDS) and the bias sums.
//   3. lane = dof in both halves, two requested roots per pass: the set of bodies of S(b) the dof moves is S(b)
//      (the dof moves b), S(body(d)) (body(d) inside S(b)) or empty, so each column is closed form on that
//      set's composite; one LDS stage per output, dyn_emit's stores.
// A body id outside 0..nbody-1 gives NaN rows. An output passed as NULL costs neither its staging nor its stores
// (branches on the kernel arguments, uniform over the wave). Every value is stored through x + 0: with qvel = 0
// the rates are +0 bit for bit.
// The subtree sums and the columns are centroidal_dev.h's (the whole-body IK kernel runs them too).
// Included by capi.hip after dyn_kernels.hip (dyn_dof_axis, dyn_emit).
#pragma once

#include "centroidal_dev.h"

namespace mjl {

struct JacDotArgs {
  const ModelF* m;      // the shared model block (no geometric field is per-env)
  const DynTab* tab;
  const float *qpos, *qvel;  // [nenv, nq], [nenv, nv]
  const float* mask;    // [nenv] or null
  int nenv, npoint, frame;
  const int32_t* body;  // [npoint]
  const float* pnt;     // MJL_JAC_WORLD [nenv, npoint, 3]; MJL_JAC_LOCAL [npoint, 3] or null
  float *jacp_dot, *jacr_dot;  // [nenv, npoint, 3, nv] each, or null
  float* jdotv;         // [nenv, npoint, 6] or null
};

struct CentArgs {
  const ModelF* m;
  const ModelF* m_env;  // [nenv] per-env blocks (MJL_OPT_PER_ENV_MODEL), or null
  const DynTab* tab;
  const float *qpos, *qvel;
  const float* mask;
  int nenv, nsub;
  const int32_t* body;  // [nsub] subtree roots
  float *jac_com, *angmom_mat;  // [nenv, nsub, 3, nv] each, or null
  float* bias;          // [nenv, nsub, 6] or null
};

// dyn_tree_pass with rates at qacc = 0: bw / bv the body's angular velocity and its origin's velocity; with ACC
// bdw / ba their velocity-product rates; with DOFR, per hinge dof, dwv / dpv: the angular velocity of the frame
// carrying the axis (the chain before the hinge) and the velocity of the anchor. Row 0 of every per-body array
// is the caller's (the world: zeros). Ends with a barrier.
template <bool DOFR, bool ACC>
static INL void ts_tree_pass(MP m, const BodyRec& br, const float* qpos, const float* qvel, float (*xpos)[3],
                             float (*xquat)[4], float (*dax)[3], float (*danc)[3], float (*dwv)[3], float (*dpv)[3],
                             float (*bw)[3], float (*bv)[3], float (*bdw)[3], float (*ba)[3], int nbody, int maxlevel,
                             int lane) {
  const bool isb = lane > 0 && lane < nbody;
  for (int L = 1; L <= maxlevel; L++) {
    if (isb && br.level == L) {
      const int par = br.parent;
      float lp[3], lq[4], w[3], v[3], dw[3] = {0.f, 0.f, 0.f}, a[3] = {0.f, 0.f, 0.f};
      if (br.isfree) {  // the world pose; local angular rates, world linear ones; d/dt (R w_local) = w x w = 0
        const int qa = br.qadr, da = max(0, min(br.dofadr, MJL_MAXV - 6));
        for (int i = 0; i < 3; i++) { lp[i] = qpos[qa + i]; v[i] = qvel[da + i]; }
        for (int i = 0; i < 4; i++) lq[i] = qpos[qa + 3 + i];
        qnorm(lq);
        float R[9];
        q2m(R, lq);
        mv3(w, R, &qvel[da + 3]);
      } else {
        float r[3], R[9];  // r: the point whose velocity and acceleration v, a are (the parent's origin at first)
        for (int i = 0; i < 3; i++) { r[i] = xpos[par][i]; w[i] = bw[par][i]; v[i] = bv[par][i]; }
        if constexpr (ACC)
          for (int i = 0; i < 3; i++) { dw[i] = bdw[par][i]; a[i] = ba[par][i]; }
        q2m(R, xquat[par]);
        mv3(lp, R, br.pos);
        for (int i = 0; i < 3; i++) lp[i] += r[i];
        qmul(lq, xquat[par], br.quat);
        for (int j = br.jntadr; j < br.jntadr + br.jntnum; j++) {
          const JntRec jr = ldrec(&m->jrec[j]);
          float anc[3], ax[3], dd[3];
          q2m(R, lq);
          mv3(anc, R, jr.pos);
          mv3(ax, R, jr.axis);
          for (int i = 0; i < 3; i++) { anc[i] += lp[i]; dd[i] = anc[i] - r[i]; r[i] = anc[i]; }
          if constexpr (ACC) move_point(v, a, w, dw, dd);
          else add_cross(v, w, dd);
          const int d = max(0, min(jr.dofadr, MJL_MAXV - 1));
          for (int i = 0; i < 3; i++) { dax[d][i] = ax[i]; danc[d][i] = anc[i]; }
          if constexpr (DOFR)
            for (int i = 0; i < 3; i++) { dwv[d][i] = w[i]; dpv[d][i] = v[i]; }
          const float qd = qvel[d];
          if constexpr (ACC) {
            float wxa[3] = {0.f, 0.f, 0.f};
            add_cross(wxa, w, ax);
            for (int i = 0; i < 3; i++) dw[i] += wxa[i] * qd;
          }
          for (int i = 0; i < 3; i++) w[i] += ax[i] * qd;
          float sn, cs;
          sincosf(0.5f * (qpos[jr.qadr] - jr.qpos0), &sn, &cs);
          const float ql[4] = {cs, jr.axis[0] * sn, jr.axis[1] * sn, jr.axis[2] * sn};
          qmul(lq, lq, ql);
          float off[3];
          q2m(R, lq);
          mv3(off, R, jr.pos);
          for (int i = 0; i < 3; i++) lp[i] = anc[i] - off[i];
        }
        qnorm(lq);
        const float dd[3] = {lp[0] - r[0], lp[1] - r[1], lp[2] - r[2]};
        if constexpr (ACC) move_point(v, a, w, dw, dd);
        else add_cross(v, w, dd);
      }
      for (int i = 0; i < 3; i++) { xpos[lane][i] = lp[i]; bw[lane][i] = w[i]; bv[lane][i] = v[i]; }
      if constexpr (ACC)
        for (int i = 0; i < 3; i++) { bdw[lane][i] = dw[i]; ba[lane][i] = a[i]; }
      for (int i = 0; i < 4; i++) xquat[lane][i] = lq[i];
    }
    __syncthreads();
  }
}

// the sum of v over the 32 lanes of the lane's half of the wave, in every lane of the half: a butterfly, one order
static INL float ts_half_sum(float v) {
  for (int k = 16; k >= 1; k >>= 1) v += __shfl_xor(v, k, 64);
  return v;
}

__global__ __launch_bounds__(64) void jac_dot_kernel(JacDotArgs A) {
  __shared__ float qpos[MJL_MAXQ], qvel[MJL_MAXV];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4], bw[MJL_MAXBODY][3], bv[MJL_MAXBODY][3];
  __shared__ float dax[MJL_MAXV][3], danc[MJL_MAXV][3], dwv[MJL_MAXV][3], dpv[MJL_MAXV][3];
  __shared__ __attribute__((aligned(16))) float stp[2 * 3 * MJL_MAXV];  // two points' jacp_dot block
  __shared__ __attribute__((aligned(16))) float str[2 * 3 * MJL_MAXV];  // and their jacr_dot block
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)A.m);
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel, npoint = A.npoint;

  if (lane < nq) qpos[lane] = A.qpos[(size_t)env * nq + lane];
  if (lane < MJL_MAXV) qvel[lane] = lane < nv ? A.qvel[(size_t)env * nv + lane] : 0.f;
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    for (int i = 0; i < 3; i++) xpos[0][i] = bw[0][i] = bv[0][i] = 0.f;
  }
  if (lane < MJL_MAXV)
    for (int i = 0; i < 3; i++) dax[lane][i] = danc[lane][i] = dwv[lane][i] = dpv[lane][i] = 0.f;
  __syncthreads();
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);
  ts_tree_pass<true, false>(m, br, qpos, qvel, xpos, xquat, dax, danc, dwv, dpv, bw, bv, nullptr, nullptr, nbody,
                            maxlevel, lane);

  // ---- lane = dof in both halves of the wave: axis, anchor and their rates
  const int d = lane & 31, h = lane >> 5;
  const bool isd = d < nv;
  const DofRec dr = ldrec(&m->drec[isd ? d : 0]);
  float ax[3], an[3], adot[3] = {0.f, 0.f, 0.f}, pdot[3] = {0.f, 0.f, 0.f};
  const int kind = dyn_dof_axis(dr, isd ? d : 0, xpos, xquat, dax, danc, nbody, ax, an);
  if (kind == 0) {
    float wf[3];  // the angular velocity of the frame carrying the axis
    if (dr.kfree < 0) {
      for (int i = 0; i < 3; i++) { wf[i] = dwv[isd ? d : 0][i]; pdot[i] = dpv[isd ? d : 0][i]; }
    } else {
      const int b = max(0, min(dr.bodyid, nbody - 1));
      for (int i = 0; i < 3; i++) { wf[i] = bw[b][i]; pdot[i] = bv[b][i]; }
    }
    add_cross(adot, wf, ax);
  }
  const float qv = isd ? qvel[d] : 0.f;
  const float nan = __int_as_float(0x7fc00000);
  const size_t blk = (size_t)3 * nv;
  const bool mats = A.jacp_dot || A.jacr_dot;

  for (int p0 = 0; p0 < npoint; p0 += 2) {
    const int p = p0 + h;
    const bool act = p < npoint;
    const int b = act ? A.body[p] : 0;
    const bool bad = b < 0 || b >= nbody;
    const int bs = bad ? 0 : b;
    float x[3] = {0.f, 0.f, 0.f};
    if (A.frame == MJL_JAC_WORLD) {
      if (act)
        for (int i = 0; i < 3; i++) x[i] = A.pnt[((size_t)env * npoint + p) * 3 + i];
    } else {
      float off[3] = {0.f, 0.f, 0.f}, R[9];
      if (A.pnt && act)
        for (int i = 0; i < 3; i++) off[i] = A.pnt[(size_t)p * 3 + i];
      q2m(R, xquat[bs]);
      mv3(x, R, off);
      for (int i = 0; i < 3; i++) x[i] += xpos[bs][i];
    }
    const bool moves = isd && ((A.tab->body_dofmask[bs] >> d) & 1u);
    float jr[3] = {0.f, 0.f, 0.f}, jp[3] = {0.f, 0.f, 0.f};
    if (moves && kind == 0) {
      // the point is fixed in its body: dx/dt = v_b + w_b x (x - xpos_b)
      const float rb[3] = {x[0] - xpos[bs][0], x[1] - xpos[bs][1], x[2] - xpos[bs][2]};
      float xd[3] = {bv[bs][0], bv[bs][1], bv[bs][2]};
      add_cross(xd, bw[bs], rb);
      const float r[3] = {x[0] - an[0], x[1] - an[1], x[2] - an[2]};
      const float rd[3] = {xd[0] - pdot[0], xd[1] - pdot[1], xd[2] - pdot[2]};
      for (int i = 0; i < 3; i++) jr[i] = adot[i];
      add_cross(jp, adot, r);
      add_cross(jp, ax, rd);
    }
    for (int i = 0; i < 3; i++) { jr[i] += 0.f; jp[i] += 0.f; }
    if (bad)
      for (int i = 0; i < 3; i++) jr[i] = jp[i] = nan;
    if (A.jdotv) {  // uniform: every lane takes part in the butterflies
      float s[6];
      for (int i = 0; i < 3; i++) { s[i] = ts_half_sum(jp[i] * qv); s[3 + i] = ts_half_sum(jr[i] * qv); }
      float mine = s[0];
      for (int i = 1; i < 6; i++) mine = d == i ? s[i] : mine;
      if (act && d < 6) A.jdotv[((size_t)env * npoint + p) * 6 + d] = bad ? nan : mine + 0.f;
    }
    if (!mats) continue;  // uniform
    if (act && isd)
      for (int i = 0; i < 3; i++) {
        if (A.jacp_dot) stp[(h * 3 + i) * nv + d] = jp[i];
        if (A.jacr_dot) str[(h * 3 + i) * nv + d] = jr[i];
      }
    __syncthreads();
    const int n = min(2, npoint - p0) * 3 * nv;
    const size_t o = ((size_t)env * npoint + p0) * blk;
    if (A.jacp_dot) dyn_emit(A.jacp_dot + o, stp, n, lane);
    if (A.jacr_dot) dyn_emit(A.jacr_dot + o, str, n, lane);
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void centroidal_kernel(CentArgs A) {
  __shared__ float qpos[MJL_MAXQ], qvel[MJL_MAXV];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float bw[MJL_MAXBODY][3], bv[MJL_MAXBODY][3], bdw[MJL_MAXBODY][3], ba[MJL_MAXBODY][3];
  __shared__ float dax[MJL_MAXV][3], danc[MJL_MAXV][3];
  __shared__ float xim[MJL_MAXBODY][4];   // xipos, mass
  __shared__ float biw[MJL_MAXBODY][6];   // the world inertia (xx yy zz xy xz yz)
  __shared__ float bmr[MJL_MAXBODY][6];   // the body's own momentum rates [m a ; I dw + w x I w]
  __shared__ float cm[MJL_MAXBODY][4];    // subtree: centre of mass, mass
  __shared__ float cI[MJL_MAXBODY][6];    // subtree: inertia about its own centre of mass
  __shared__ float sb[MJL_MAXBODY][6];    // subtree: the bias [sum m a / mass ; d/dt angular momentum]
  __shared__ int ssend[MJL_MAXBODY];
  __shared__ __attribute__((aligned(16))) float stp[2 * 3 * MJL_MAXV];  // two roots' jac_com block
  __shared__ __attribute__((aligned(16))) float str[2 * 3 * MJL_MAXV];  // and their angmom_mat block
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel, nsub = A.nsub;
  const bool mats = A.jac_com || A.angmom_mat;

  if (lane < nq) qpos[lane] = A.qpos[(size_t)env * nq + lane];
  if (lane < MJL_MAXV) qvel[lane] = lane < nv ? A.qvel[(size_t)env * nv + lane] : 0.f;
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    for (int i = 0; i < 3; i++) xpos[0][i] = bw[0][i] = bv[0][i] = bdw[0][i] = ba[0][i] = 0.f;
  }
  if (lane < MJL_MAXV)
    for (int i = 0; i < 3; i++) dax[lane][i] = danc[lane][i] = 0.f;
  __syncthreads();
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);
  ts_tree_pass<false, true>(m, br, qpos, qvel, xpos, xquat, dax, danc, nullptr, nullptr, bw, bv, bdw, ba, nbody,
                            maxlevel, lane);

  // ---- lane = body: the inertial frame's origin, the world inertia, the momentum rates (row 0, the world: zeros)
  float xi[3] = {0.f, 0.f, 0.f}, IW[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float mr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float mass = isb ? br.mass : 0.f;
  if (isb) {
    float R[9], dd[3], vc[3], ac[3], w[3], dw[3];
    q2m(R, xquat[lane]);
    mv3(dd, R, br.ipos);
    for (int i = 0; i < 3; i++) { xi[i] = xpos[lane][i] + dd[i]; vc[i] = bv[lane][i]; ac[i] = ba[lane][i]; w[i] = bw[lane][i]; dw[i] = bdw[lane][i]; }
    move_point(vc, ac, w, dw, dd);
    const float* t = br.inertia;
    const float T[9] = {t[0], t[3], t[4], t[3], t[1], t[5], t[4], t[5], t[2]};
    float RT[9];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) RT[3 * i + k] = R[3 * i] * T[k] + R[3 * i + 1] * T[3 + k] + R[3 * i + 2] * T[6 + k];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) IW[3 * i + k] = RT[3 * i] * R[3 * k] + RT[3 * i + 1] * R[3 * k + 1] + RT[3 * i + 2] * R[3 * k + 2];
    float Iwv[3];
    mv3(Iwv, IW, w);
    mv3(mr + 3, IW, dw);
    add_cross(mr + 3, w, Iwv);
    for (int i = 0; i < 3; i++) mr[i] = mass * ac[i];
  }
  const int send = lane < nbody ? max(lane + 1, min(br.subtree_end, nbody)) : 0;
  if (lane < nbody) {
    for (int i = 0; i < 3; i++) xim[lane][i] = xi[i];
    xim[lane][3] = mass;
    biw[lane][0] = IW[0]; biw[lane][1] = IW[4]; biw[lane][2] = IW[8];
    biw[lane][3] = IW[1]; biw[lane][4] = IW[2]; biw[lane][5] = IW[5];
    for (int i = 0; i < 6; i++) bmr[lane][i] = mr[i];
    ssend[lane] = send;
  }
  __syncthreads();

  // ---- lane = subtree root s: the composite of [s, subtree_end) about its own centre of mass, and its bias
  if (lane < nbody) {
    float ms, inv, c[3];
    bool empty;  // a massless subtree: its own xipos, zero rows
    cent_subtree_com(xim, lane, send, xi, c, ms, inv, empty);
    float I6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, F[3] = {0.f, 0.f, 0.f}, T[3] = {0.f, 0.f, 0.f};
    for (int k = lane; k < send; k++) {
      const float mk = xim[k][3];
      const float r[3] = {xim[k][0] - c[0], xim[k][1] - c[1], xim[k][2] - c[2]};
      if (A.angmom_mat) {
        const float rr = dot3(r, r);
        I6[0] += biw[k][0] + mk * (rr - r[0] * r[0]); I6[1] += biw[k][1] + mk * (rr - r[1] * r[1]);
        I6[2] += biw[k][2] + mk * (rr - r[2] * r[2]);
        I6[3] += biw[k][3] - mk * r[0] * r[1]; I6[4] += biw[k][4] - mk * r[0] * r[2]; I6[5] += biw[k][5] - mk * r[1] * r[2];
      }
      if (A.bias) {
        const float f[3] = {bmr[k][0], bmr[k][1], bmr[k][2]};
        for (int i = 0; i < 3; i++) { F[i] += f[i]; T[i] += bmr[k][3 + i]; }
        add_cross(T, r, f);
      }
    }
    for (int i = 0; i < 3; i++) cm[lane][i] = c[i];
    cm[lane][3] = empty ? 0.f : ms;
    for (int i = 0; i < 6; i++) cI[lane][i] = empty ? 0.f : I6[i];
    for (int i = 0; i < 3; i++) { sb[lane][i] = F[i] * inv + 0.f; sb[lane][3 + i] = empty ? 0.f : T[i] + 0.f; }
  }
  __syncthreads();

  const float nan = __int_as_float(0x7fc00000);
  if (A.bias && lane < nsub) {
    const int b = A.body[lane];
    const bool bad = b < 0 || b >= nbody;
    for (int i = 0; i < 6; i++) A.bias[((size_t)env * nsub + lane) * 6 + i] = bad ? nan : sb[b][i];
  }
  if (!mats) return;  // uniform

  // ---- lane = dof in both halves of the wave, two roots per pass
  const int d = lane & 31, h = lane >> 5;
  const bool isd = d < nv;
  const DofRec dr = ldrec(&m->drec[isd ? d : 0]);
  float ax[3], an[3];
  const int kind = dyn_dof_axis(dr, isd ? d : 0, xpos, xquat, dax, danc, nbody, ax, an);
  const int db = max(0, min(dr.bodyid, nbody - 1));
  const size_t blk = (size_t)3 * nv;

  for (int p0 = 0; p0 < nsub; p0 += 2) {
    const int p = p0 + h;
    const bool act = p < nsub;
    const int b = act ? A.body[p] : 0;
    const bool bad = b < 0 || b >= nbody;
    const int bs = bad ? 0 : b;
    // the bodies of S(bs) that dof d moves: all of it, the subtree of the dof's body, or none
    const int S = cent_moved_set(A.tab, bs, d, db, ssend, isd);
    float jc[3], am[3];
    cent_column<true>(S, bs, cm, cI, kind, ax, an, jc, am);
    for (int i = 0; i < 3; i++) { jc[i] += 0.f; am[i] += 0.f; }
    if (bad)
      for (int i = 0; i < 3; i++) jc[i] = am[i] = nan;
    if (act && isd)
      for (int i = 0; i < 3; i++) {
        if (A.jac_com) stp[(h * 3 + i) * nv + d] = jc[i];
        if (A.angmom_mat) str[(h * 3 + i) * nv + d] = am[i];
      }
    __syncthreads();
    const int n = min(2, nsub - p0) * 3 * nv;
    const size_t o = ((size_t)env * nsub + p0) * blk;
    if (A.jac_com) dyn_emit(A.jac_com + o, stp, n, lane);
    if (A.angmom_mat) dyn_emit(A.angmom_mat + o, str, n, lane);
    __syncthreads();
  }
}

}  // namespace mjl
