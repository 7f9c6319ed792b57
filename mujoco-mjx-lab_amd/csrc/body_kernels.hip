// Body-level Data readout (mjl_body_data): xipos, ximat, subtree_com, cinert, cvel, subtree_linvel,
// subtree_angmom, cfrc_ext and cfrc_int of the batch's current state, as include/mjx355.h defines them.
//
// A kernel of its own with a workspace of its own (6.6 KB of LDS): nothing of the step kernel's workspace or
// phases is touched and none of its out-of-line functions is called from here. One wavefront per env, lane =
// body (MJL_MAXBODY = 32 <= 64). D is only the row stride of the env's global row slab (global_rows<D>), read
// for the contacts of cfrc_ext.
//   1. qpos, qvel (and, for the cfrc outputs, the forward pass's qacc) into LDS.
//   2. The tree pass of sensors_kernel, restated (sensor_kernels.hip has the derivation): frame, w, dw/dt and
//      the origin's v, a of every body, a level at a time.
//   3. Lane = body: xipos, the centre of mass's velocity and acceleration (move_point by R ipos), the world
//      inertia R T R' from the body-frame tensor T, and I w; xipos, mass, the velocity and I w into LDS.
//   4. Lane = b, one loop over its contiguous subtree [b, subtree_end) out of LDS: mass, sum m xipos, sum m v
//      -> subtree_com, subtree_linvel; a second loop for the angular momentum about that centre.
//   5. With c0 = subtree_com[rootid]: cinert, cvel; for the cfrc outputs the external wrench about c0 (the
//      body's xfrc_applied row, then one wave-uniform loop over the env's contacts in contact order: a fixed
//      summation order, no atomics) and the body's net wrench [I dw + w x I w + r x f ; f] - cfrc_ext into LDS,
//      f = m (a - g); cfrc_int[b] is its sum over the subtree.
//   6. Every requested output: the rows into one LDS stage, then consecutive lanes store consecutive floats of
//      the env's contiguous [nbody, k] block (b128 when the block is 16-byte aligned and a multiple of 4 floats).
// An output that is not requested costs neither its arithmetic nor its stores (branches on the kernel
// arguments, uniform over the wave).
// Included by capi.hip after sensor_kernels.hip (small math, ldrec, add_cross / move_point, contact_frame_force).
#pragma once

namespace mjl {

struct BodyArgs {
  const ModelF* m;        // the shared model block
  const ModelF* m_env;    // [nenv] per-env blocks (MJL_OPT_PER_ENV_MODEL), or null
  const BodyTab* tab;
  StateBuf s;
  const float* mask;      // [nenv] or null
  const float* xfrc;      // the attached xfrc_applied [nenv, nbody, 6], or null (read for the cfrc outputs only)
  float* scratch;         // the global row slabs (read for the cfrc outputs only)
  int scratch_stride, gmax_efc, gmax_con;
  int nenv;
  // [nenv, nbody, k] each, or null: k = 3, 9, 3, 10, 6, 3, 3, 6, 6
  float *xipos, *ximat, *subtree_com, *cinert, *cvel, *subtree_linvel, *subtree_angmom, *cfrc_ext, *cfrc_int;
};

// rows [nbody][K] of one output: lane b's row into the stage, then the env's block out
template <int K>
static INL void body_emit(float* out, float* stage, const float (&val)[K], int nbody, int lane, int env) {
  if (lane < nbody)
    for (int i = 0; i < K; i++) stage[lane * K + i] = val[i];
  __syncthreads();
  const int n = nbody * K;
  float* o = out + (size_t)env * (size_t)n;
  if ((n & 3) == 0 && ((uintptr_t)o & 15) == 0) {
    for (int i = lane; i < n / 4; i += 64) ((f32x4*)o)[i] = ((const f32x4*)stage)[i];
  } else {
    for (int i = lane; i < n; i += 64) o[i] = stage[i];
  }
  __syncthreads();
}

template <class D>
__global__ __launch_bounds__(64) void body_data_kernel(BodyArgs A) {
  __shared__ float qpos[MJL_MAXQ], qvel[MJL_MAXV], qacc[MJL_MAXV];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float bw[MJL_MAXBODY][3], bdw[MJL_MAXBODY][3], bv[MJL_MAXBODY][3], ba[MJL_MAXBODY][3];
  __shared__ float xim[MJL_MAXBODY][4];                         // xipos, mass
  __shared__ float vcm[MJL_MAXBODY][3], Iw[MJL_MAXBODY][3];     // the centre of mass's velocity; I w
  __shared__ float scom[MJL_MAXBODY][3];                        // subtree_com
  __shared__ float wr[MJL_MAXBODY][6];                          // net wrench about c0 minus cfrc_ext
  __shared__ __attribute__((aligned(16))) float stage[MJL_MAXBODY * 10];
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));
  const bool acc = A.cfrc_ext || A.cfrc_int;
  const bool mom = A.subtree_linvel || A.subtree_angmom;
  const bool sub = A.subtree_com || A.cinert || A.cvel || mom || acc;  // the subtree centres of mass are needed
  const bool inert = A.cinert || A.subtree_angmom || A.cfrc_int;      // the world inertia is needed
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel;

  if (lane < nq) qpos[lane] = A.s.qpos[(size_t)env * nq + lane];
  if (lane < nv) {
    qvel[lane] = A.s.qvel[(size_t)env * nv + lane];
    qacc[lane] = acc ? A.s.qacc[(size_t)env * nv + lane] : 0.f;
  }
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    for (int i = 0; i < 3; i++) xpos[0][i] = bw[0][i] = bdw[0][i] = bv[0][i] = ba[0][i] = 0.f;
  }
  __syncthreads();

  // ---- tree pass: frames and rates of every body, a level at a time (as sensors_kernel)
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);
  for (int L = 1; L <= maxlevel; L++) {
    if (isb && br.level == L) {
      const int par = br.parent;
      float lp[3], lq[4], w[3], dw[3], v[3], a[3];
      if (br.isfree) {  // the world pose; local angular rates, world linear ones
        const int qa = br.qadr, da = br.dofadr;
        for (int i = 0; i < 3; i++) { lp[i] = qpos[qa + i]; v[i] = qvel[da + i]; a[i] = qacc[da + i]; }
        for (int i = 0; i < 4; i++) lq[i] = qpos[qa + 3 + i];
        qnorm(lq);
        float R[9];
        q2m(R, lq);
        mv3(w, R, &qvel[da + 3]);
        mv3(dw, R, &qacc[da + 3]);
      } else {
        float r[3], R[9];  // r: the point whose velocity and acceleration v, a are (the parent's origin at first)
        for (int i = 0; i < 3; i++) { r[i] = xpos[par][i]; w[i] = bw[par][i]; dw[i] = bdw[par][i]; v[i] = bv[par][i]; a[i] = ba[par][i]; }
        q2m(R, xquat[par]);
        mv3(lp, R, br.pos);
        for (int i = 0; i < 3; i++) lp[i] += r[i];
        qmul(lq, xquat[par], br.quat);
        for (int j = br.jntadr; j < br.jntadr + br.jntnum; j++) {
          const JntRec jr = ldrec(&m->jrec[j]);
          float anc[3], ax[3], d[3];
          q2m(R, lq);
          mv3(anc, R, jr.pos);
          mv3(ax, R, jr.axis);
          for (int i = 0; i < 3; i++) { anc[i] += lp[i]; d[i] = anc[i] - r[i]; r[i] = anc[i]; }
          move_point(v, a, w, dw, d);
          const float qd = qvel[jr.dofadr], qdd = qacc[jr.dofadr];
          float wxa[3] = {0.f, 0.f, 0.f};
          add_cross(wxa, w, ax);
          for (int i = 0; i < 3; i++) { dw[i] += ax[i] * qdd + wxa[i] * qd; w[i] += ax[i] * qd; }
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
        const float d[3] = {lp[0] - r[0], lp[1] - r[1], lp[2] - r[2]};
        move_point(v, a, w, dw, d);
      }
      for (int i = 0; i < 3; i++) { xpos[lane][i] = lp[i]; bw[lane][i] = w[i]; bdw[lane][i] = dw[i]; bv[lane][i] = v[i]; ba[lane][i] = a[i]; }
      for (int i = 0; i < 4; i++) xquat[lane][i] = lq[i];
    }
    __syncthreads();
  }

  // ---- lane = body: the inertial frame's origin and its rates, the world inertia (row 0, the world: zeros)
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  float xi[3] = {0.f, 0.f, 0.f}, vc[3] = {0.f, 0.f, 0.f}, ac[3] = {0.f, 0.f, 0.f};
  float w[3] = {0.f, 0.f, 0.f}, dw[3] = {0.f, 0.f, 0.f}, IW[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float Iwv[3] = {0.f, 0.f, 0.f};
  const float mass = isb ? br.mass : 0.f;
  if (isb) {
    float d[3];
    q2m(R, xquat[lane]);
    mv3(d, R, br.ipos);
    for (int i = 0; i < 3; i++) { xi[i] = xpos[lane][i] + d[i]; vc[i] = bv[lane][i]; ac[i] = ba[lane][i]; w[i] = bw[lane][i]; dw[i] = bdw[lane][i]; }
    move_point(vc, ac, w, dw, d);
    if (inert) {  // R T R', T the body-frame tensor (xx yy zz xy xz yz)
      const float* t = br.inertia;
      const float T[9] = {t[0], t[3], t[4], t[3], t[1], t[5], t[4], t[5], t[2]};
      float RT[9];
      for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) RT[3 * i + k] = R[3 * i] * T[k] + R[3 * i + 1] * T[3 + k] + R[3 * i + 2] * T[6 + k];
      for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) IW[3 * i + k] = RT[3 * i] * R[3 * k] + RT[3 * i + 1] * R[3 * k + 1] + RT[3 * i + 2] * R[3 * k + 2];
      mv3(Iwv, IW, w);
    }
  }
  if (lane < nbody) {
    for (int i = 0; i < 3; i++) { xim[lane][i] = xi[i]; vcm[lane][i] = vc[i]; Iw[lane][i] = Iwv[i]; }
    xim[lane][3] = mass;
  }
  if (A.xipos) body_emit<3>(A.xipos, stage, xi, nbody, lane, env);
  if (A.ximat) {  // xmat quat2mat(body_iquat), row-major (row 0: the identity)
    float Ri[9], XI[9];
    q2m(Ri, A.tab->iquat[lane < nbody ? lane : 0]);
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) XI[3 * i + k] = R[3 * i] * Ri[k] + R[3 * i + 1] * Ri[3 + k] + R[3 * i + 2] * Ri[6 + k];
    body_emit<9>(A.ximat, stage, XI, nbody, lane, env);
  }
  if (!sub) return;  // uniform: nothing past the per-body frames was asked for
  __syncthreads();

  // ---- lane = b: sums over the subtree [b, subtree_end)
  const int send = lane < nbody ? max(lane + 1, min(br.subtree_end, nbody)) : 0;
  float cb[3] = {0.f, 0.f, 0.f}, lv[3] = {0.f, 0.f, 0.f}, am[3] = {0.f, 0.f, 0.f};
  if (lane < nbody) {
    float ms = 0.f, s[3] = {0.f, 0.f, 0.f}, p[3] = {0.f, 0.f, 0.f};
    for (int k = lane; k < send; k++) {
      const float mk = xim[k][3];
      ms += mk;
      for (int i = 0; i < 3; i++) s[i] += mk * xim[k][i];
      if (mom)
        for (int i = 0; i < 3; i++) p[i] += mk * vcm[k][i];
    }
    const bool empty = ms < kMinVal;  // a massless subtree: its own xipos, no momentum
    const float inv = empty ? 0.f : 1.f / ms;
    for (int i = 0; i < 3; i++) { cb[i] = empty ? xi[i] : s[i] * inv; lv[i] = p[i] * inv; }
    if (A.subtree_angmom) {
      for (int k = lane; k < send; k++) {
        const float mk = xim[k][3];
        const float dx[3] = {xim[k][0] - cb[0], xim[k][1] - cb[1], xim[k][2] - cb[2]};
        const float dv[3] = {mk * (vcm[k][0] - lv[0]), mk * (vcm[k][1] - lv[1]), mk * (vcm[k][2] - lv[2])};
        for (int i = 0; i < 3; i++) am[i] += Iw[k][i];
        add_cross(am, dx, dv);
      }
    }
    for (int i = 0; i < 3; i++) scom[lane][i] = cb[i];
  }
  if (A.subtree_com) body_emit<3>(A.subtree_com, stage, cb, nbody, lane, env);
  if (A.subtree_linvel) body_emit<3>(A.subtree_linvel, stage, lv, nbody, lane, env);
  if (A.subtree_angmom) body_emit<3>(A.subtree_angmom, stage, am, nbody, lane, env);
  if (!(A.cinert || A.cvel || acc)) return;
  __syncthreads();

  // ---- about c0, the centre of mass of the body's kinematic tree
  float r[3] = {0.f, 0.f, 0.f}, c0[3] = {0.f, 0.f, 0.f};
  if (isb) {
    const int root = max(0, min(br.rootid, nbody - 1));
    for (int i = 0; i < 3; i++) { c0[i] = scom[root][i]; r[i] = xi[i] - c0[i]; }
  }
  if (A.cinert) {
    float ci[10];
    const float rr = dot3(r, r);
    ci[0] = IW[0] + mass * (rr - r[0] * r[0]); ci[1] = IW[4] + mass * (rr - r[1] * r[1]); ci[2] = IW[8] + mass * (rr - r[2] * r[2]);
    ci[3] = IW[1] - mass * r[0] * r[1]; ci[4] = IW[2] - mass * r[0] * r[2]; ci[5] = IW[5] - mass * r[1] * r[2];
    ci[6] = mass * r[0]; ci[7] = mass * r[1]; ci[8] = mass * r[2]; ci[9] = mass;
    body_emit<10>(A.cinert, stage, ci, nbody, lane, env);
  }
  if (A.cvel) {  // the body-fixed point at c0: v_c0 = v_com + w x (c0 - xipos)
    float cv[6] = {w[0], w[1], w[2], vc[0], vc[1], vc[2]};
    const float mr[3] = {-r[0], -r[1], -r[2]};
    add_cross(cv + 3, w, mr);
    body_emit<6>(A.cvel, stage, cv, nbody, lane, env);
  }
  if (!acc) return;

  // ---- external wrench on the body alone: its xfrc_applied row, then the contacts in contact order
  float ext[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (isb && A.xfrc) {
    const float* x = A.xfrc + ((size_t)env * nbody + lane) * 6;
    const float f[3] = {x[0], x[1], x[2]};
    for (int i = 0; i < 3; i++) { ext[i] = x[3 + i]; ext[3 + i] = f[i]; }
    add_cross(ext, r, f);
  }
  {
    const Rows<true> Rw = global_rows<D>(A.scratch + (size_t)env * (size_t)A.scratch_stride, A.gmax_efc, A.gmax_con);
    const int nslab = max(0, min(uni_int((int)A.s.stats[(size_t)env * 4]), A.gmax_con));
    for (int c = 0; c < nslab; c++) {  // uniform: every lane reads the same contact
      const GLBA float* cr = Rw.con + c * CONW;
      const int packed = __float_as_int(cr[15]), dim = (packed >> 16) & 0xff;
      const int b1 = packed & 0xff, b2 = (packed >> 8) & 0xff;
      float f[3], F[3];
      contact_frame_force(Rw, contact_row0(Rw, c, dim), dim, cr[14], f);
      for (int k = 0; k < 3; k++) F[k] = cr[3 + k] * f[0] + cr[6 + k] * f[1] + cr[9 + k] * f[2];
      if (isb && (lane == b1 || lane == b2)) {  // +F on geom2's body, -F on geom1's, at the contact's pos
        if (lane == b1)
          for (int k = 0; k < 3; k++) F[k] = -F[k];
        const float rc[3] = {cr[0] - c0[0], cr[1] - c0[1], cr[2] - c0[2]};
        add_cross(ext, rc, F);
        for (int k = 0; k < 3; k++) ext[3 + k] += F[k];
      }
    }
  }
  if (lane < nbody) {
    float f[3], t[3], IdW[3];
    for (int i = 0; i < 3; i++) f[i] = mass * (ac[i] - m->gravity[i]);
    mv3(IdW, IW, dw);
    for (int i = 0; i < 3; i++) t[i] = IdW[i];
    add_cross(t, w, Iwv);
    add_cross(t, r, f);
    for (int i = 0; i < 3; i++) { wr[lane][i] = t[i] - ext[i]; wr[lane][3 + i] = f[i] - ext[3 + i]; }
  }
  if (A.cfrc_ext) body_emit<6>(A.cfrc_ext, stage, ext, nbody, lane, env);
  if (A.cfrc_int) {
    __syncthreads();
    float ci[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (isb)
      for (int k = lane; k < send; k++)
        for (int i = 0; i < 6; i++) ci[i] += wr[k][i];
    body_emit<6>(A.cfrc_int, stage, ci, nbody, lane, env);
  }
}

}  // namespace mjl
