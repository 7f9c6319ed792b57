// Jacobian and mass-matrix readout (mjl_jac, mjl_mass_matrix): point Jacobians jacp / jacr of bodies and sites,
// the dense joint-space inertia M of the batch's current qpos, M v and M^-1 v, as include/mjx355.h defines them.
//
// Two kernels of their own, each with a workspace of its own (jac_kernel 3.3 KB of LDS, mass_matrix_kernel
// 10.8 KB): nothing of the step kernel's workspace or phases is touched and none of its out-of-line functions
// is called from here. One wavefront per env. Both start with the same positions-only tree pass
// (dyn_tree_pass: body_data_kernel's, without the rates), which also keeps the world axis and anchor of every
// hinge dof in LDS.
//
// jac_kernel
//   1. qpos into LDS; the tree pass; lane = dof (both halves of the wave, d = lane & 31): the dof's world axis
//      and anchor into registers (a hinge's out of LDS, a free rotation's R_b e_i about xpos_b, a free
//      translation's e_i).
//   2. Points two at a time, the lower half of the wave taking point p and the upper half p + 1: the world
//      point x (MJL_JAC_WORLD: read; MJL_JAC_LOCAL: xpos_b + R_b offset), the body's dof mask out of DynTab,
//      column d of jacr (the axis) and jacp (axis x (x - anchor)) or zeros, into one LDS stage per output;
//      then consecutive lanes store consecutive floats of the two points' contiguous 2 x 3 x nv block (b128
//      when the block is 16-byte aligned and a multiple of 4 floats). xpnt: three lanes of each half.
//   A body id outside 0..nbody-1 gives NaN rows (mjl_gather_rows' rule). An output passed as NULL costs
//   neither its staging nor its stores (branches on the kernel arguments, uniform over the wave).
//
// mass_matrix_kernel (env e on its own model block while per-env model parameters are on)
//   1. qpos into LDS; the tree pass.
//   2. lane = body: xipos, the world inertia R T R'; the subtree centres of mass (one loop over the contiguous
//      subtree out of LDS); cinert about c0 = subtree_com[rootid] (body_data_kernel's expressions); crb[b] =
//      sum of cinert over subtree(b).
//   3. lane = dof: cdof_d = [axis ; axis x (c0 - anchor)] and f_d = crb[body(d)] cdof_d into LDS.
//   4. lane = row i, the row in registers: M[i][j] = cdof_a . f_b with (a, b) = (j, i) when j is i or one of its
//      ancestors (DofRec.ancmask), (i, j) when j is a descendant (dof_descmask), else 0; armature on the
//      diagonal. Both triangles come from one fma chain over the same operands, so M is symmetric bit for bit.
//      Rows / columns past nv are the identity's.
//   5. full_m: the rows into the LDS stage (stride 33), then consecutive lanes store consecutive floats of the
//      env's [nv, nv] block. mul_m: y_i = sum_j M[i][j] v_j, v_j by readlane.
//   6. solve_m: the right-looking Cholesky factor on the rows in registers (one readlane broadcast and one fma
//      per element), L through the LDS stage into column registers as well, then per vector the forward
//      substitution on the rows and the back substitution on the columns, one readlane and one fma per step.
// Included by capi.hip after body_kernels.hip (small math, ldrec, add_cross).
#pragma once

namespace mjl {

struct JacArgs {
  const ModelF* m;      // the shared model block (no geometric field is per-env)
  const DynTab* tab;
  const float* qpos;    // [nenv, nq]
  const float* mask;    // [nenv] or null
  int nenv, npoint, frame;
  const int32_t* body;  // [npoint]
  const float* pnt;     // MJL_JAC_WORLD [nenv, npoint, 3]; MJL_JAC_LOCAL [npoint, 3] or null
  float *jacp, *jacr;   // [nenv, npoint, 3, nv] each, or null
  float* xpnt;          // [nenv, npoint, 3] or null
};

struct MassArgs {
  const ModelF* m;
  const ModelF* m_env;  // [nenv] per-env blocks (MJL_OPT_PER_ENV_MODEL), or null
  const float* qpos;
  const float* mask;
  int nenv, nvec;
  const float* vec;     // [nenv, nvec, nv] or null
  float* full_m;        // [nenv, nv, nv] or null
  float *mul_m, *solve_m;  // [nenv, nvec, nv] each, or null
};

constexpr int kDynLD = MJL_MAXV + 1;  // row stride of the matrix stage: rows and columns both conflict-free
static_assert(MJL_MAXV == 32 && MJL_MAXBODY <= 32 && MJL_MAXQ <= 64, "lane = dof in each half of the wave");

// Frames of every body from qpos (LDS), a level at a time, and the world axis / anchor of every hinge dof.
// Row 0 of xpos / xquat is the caller's (the world frame). Ends with a barrier.
static INL void dyn_tree_pass(MP m, const BodyRec& br, const float* qpos, float (*xpos)[3], float (*xquat)[4],
                              float (*dax)[3], float (*danc)[3], int nbody, int maxlevel, int lane) {
  const bool isb = lane > 0 && lane < nbody;
  for (int L = 1; L <= maxlevel; L++) {
    if (isb && br.level == L) {
      const int par = br.parent;
      float lp[3], lq[4];
      if (br.isfree) {
        const int qa = br.qadr;
        for (int i = 0; i < 3; i++) lp[i] = qpos[qa + i];
        for (int i = 0; i < 4; i++) lq[i] = qpos[qa + 3 + i];
        qnorm(lq);
      } else {
        float R[9];
        q2m(R, xquat[par]);
        mv3(lp, R, br.pos);
        for (int i = 0; i < 3; i++) lp[i] += xpos[par][i];
        qmul(lq, xquat[par], br.quat);
        for (int j = br.jntadr; j < br.jntadr + br.jntnum; j++) {
          const JntRec jr = ldrec(&m->jrec[j]);
          float anc[3], ax[3];
          q2m(R, lq);
          mv3(anc, R, jr.pos);
          mv3(ax, R, jr.axis);
          for (int i = 0; i < 3; i++) anc[i] += lp[i];
          const int d = max(0, min(jr.dofadr, MJL_MAXV - 1));
          for (int i = 0; i < 3; i++) { dax[d][i] = ax[i]; danc[d][i] = anc[i]; }
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
      }
      for (int i = 0; i < 3; i++) xpos[lane][i] = lp[i];
      for (int i = 0; i < 4; i++) xquat[lane][i] = lq[i];
    }
    __syncthreads();
  }
}

// the world axis and anchor of dof d: kind 0 a rotation about `ax` through `an`, 1 a translation along ax
static INL int dyn_dof_axis(const DofRec& dr, int d, float (*xpos)[3], float (*xquat)[4], float (*dax)[3],
                            float (*danc)[3], int nbody, float* ax, float* an) {
  const int k = dr.kfree;
  if (k < 0) {
    for (int i = 0; i < 3; i++) { ax[i] = dax[d][i]; an[i] = danc[d][i]; }
    return 0;
  }
  const int b = max(0, min(dr.bodyid, nbody - 1));
  for (int i = 0; i < 3; i++) an[i] = xpos[b][i];
  if (k < 3) {
    for (int i = 0; i < 3; i++) ax[i] = i == k ? 1.f : 0.f;
    return 1;
  }
  float R[9];
  q2m(R, xquat[b]);
  for (int i = 0; i < 3; i++) ax[i] = k == 3 ? R[3 * i] : (k == 4 ? R[3 * i + 1] : R[3 * i + 2]);  // column k - 3
  return 0;
}

// n floats of the stage to o, consecutive lanes on consecutive floats
static INL void dyn_emit(float* o, const float* stage, int n, int lane) {
  if ((n & 3) == 0 && ((uintptr_t)o & 15) == 0) {
    for (int i = lane; i < n / 4; i += 64) ((f32x4*)o)[i] = ((const f32x4*)stage)[i];
  } else {
    for (int i = lane; i < n; i += 64) o[i] = stage[i];
  }
}

__global__ __launch_bounds__(64) void jac_kernel(JacArgs A) {
  __shared__ float qpos[MJL_MAXQ];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float dax[MJL_MAXV][3], danc[MJL_MAXV][3];
  __shared__ __attribute__((aligned(16))) float stp[2 * 3 * MJL_MAXV];  // two points' jacp block
  __shared__ __attribute__((aligned(16))) float str[2 * 3 * MJL_MAXV];  // and their jacr block
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)A.m);
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel, npoint = A.npoint;

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

  // ---- lane = dof in both halves of the wave
  const int d = lane & 31, h = lane >> 5;
  const bool isd = d < nv;
  const DofRec dr = ldrec(&m->drec[isd ? d : 0]);
  float ax[3], an[3];
  const int kind = dyn_dof_axis(dr, isd ? d : 0, xpos, xquat, dax, danc, nbody, ax, an);
  const float nan = __int_as_float(0x7fc00000);
  const size_t blk = (size_t)3 * nv;

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
    if (moves) {
      if (kind == 1) {
        for (int i = 0; i < 3; i++) jp[i] = ax[i];
      } else {
        const float r[3] = {x[0] - an[0], x[1] - an[1], x[2] - an[2]};
        for (int i = 0; i < 3; i++) jr[i] = ax[i];
        add_cross(jp, ax, r);
      }
    }
    if (bad)
      for (int i = 0; i < 3; i++) jr[i] = jp[i] = x[i] = nan;
    if (act && isd)
      for (int i = 0; i < 3; i++) {
        if (A.jacp) stp[(h * 3 + i) * nv + d] = jp[i];
        if (A.jacr) str[(h * 3 + i) * nv + d] = jr[i];
      }
    if (A.xpnt && act && d < 3) A.xpnt[((size_t)env * npoint + p) * 3 + d] = d == 0 ? x[0] : (d == 1 ? x[1] : x[2]);
    __syncthreads();
    const int n = min(2, npoint - p0) * 3 * nv;
    const size_t o = ((size_t)env * npoint + p0) * blk;
    if (A.jacp) dyn_emit(A.jacp + o, stp, n, lane);
    if (A.jacr) dyn_emit(A.jacr + o, str, n, lane);
    __syncthreads();
  }
}

static INL float dyn_dot6(const float* a, const float* b) {
  return fmaf(a[5], b[5], fmaf(a[4], b[4], fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])))));
}

__global__ __launch_bounds__(64) void mass_matrix_kernel(MassArgs A) {
  constexpr int NV = MJL_MAXV, LD = kDynLD;
  __shared__ float qpos[MJL_MAXQ];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float dax[NV][3], danc[NV][3];
  __shared__ float xim[MJL_MAXBODY][4];   // xipos, mass
  __shared__ float scom[MJL_MAXBODY][3];  // subtree_com
  __shared__ float cinert[MJL_MAXBODY][10], crb[MJL_MAXBODY][10];
  __shared__ float cdof[NV][6], fd[NV][6];
  __shared__ float Ms[NV * LD];           // the matrix stage: M's rows out, then L's rows in for its columns
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, maxlevel = m->maxlevel, nvec = A.nvec;

  if (lane < nq) qpos[lane] = A.qpos[(size_t)env * nq + lane];
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    xpos[0][0] = xpos[0][1] = xpos[0][2] = 0.f;
  }
  if (lane < NV)
    for (int i = 0; i < 3; i++) dax[lane][i] = danc[lane][i] = 0.f;
  __syncthreads();
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[lane < nbody ? lane : 0]);
  dyn_tree_pass(m, br, qpos, xpos, xquat, dax, danc, nbody, maxlevel, lane);

  // ---- lane = body: the inertial frame's origin, the world inertia (row 0, the world: zeros)
  float xi[3] = {0.f, 0.f, 0.f}, IW[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const float mass = isb ? br.mass : 0.f;
  if (isb) {
    float R[9], dd[3];
    q2m(R, xquat[lane]);
    mv3(dd, R, br.ipos);
    for (int i = 0; i < 3; i++) xi[i] = xpos[lane][i] + dd[i];
    const float* t = br.inertia;
    const float T[9] = {t[0], t[3], t[4], t[3], t[1], t[5], t[4], t[5], t[2]};
    float RT[9];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) RT[3 * i + k] = R[3 * i] * T[k] + R[3 * i + 1] * T[3 + k] + R[3 * i + 2] * T[6 + k];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) IW[3 * i + k] = RT[3 * i] * R[3 * k] + RT[3 * i + 1] * R[3 * k + 1] + RT[3 * i + 2] * R[3 * k + 2];
  }
  if (lane < nbody) {
    for (int i = 0; i < 3; i++) xim[lane][i] = xi[i];
    xim[lane][3] = mass;
  }
  __syncthreads();
  const int send = lane < nbody ? max(lane + 1, min(br.subtree_end, nbody)) : 0;
  if (lane < nbody) {  // the centre of mass of the subtree [b, subtree_end)
    float ms = 0.f, s[3] = {0.f, 0.f, 0.f};
    for (int k = lane; k < send; k++) {
      const float mk = xim[k][3];
      ms += mk;
      for (int i = 0; i < 3; i++) s[i] += mk * xim[k][i];
    }
    const bool empty = ms < kMinVal;
    const float inv = empty ? 0.f : 1.f / ms;
    for (int i = 0; i < 3; i++) scom[lane][i] = empty ? xi[i] : s[i] * inv;
  }
  __syncthreads();
  if (lane < nbody) {  // cinert about c0, the centre of mass of the body's kinematic tree
    float r[3] = {0.f, 0.f, 0.f};
    if (isb) {
      const int root = max(0, min(br.rootid, nbody - 1));
      for (int i = 0; i < 3; i++) r[i] = xi[i] - scom[root][i];
    }
    const float rr = dot3(r, r);
    float* ci = cinert[lane];
    ci[0] = IW[0] + mass * (rr - r[0] * r[0]); ci[1] = IW[4] + mass * (rr - r[1] * r[1]); ci[2] = IW[8] + mass * (rr - r[2] * r[2]);
    ci[3] = IW[1] - mass * r[0] * r[1]; ci[4] = IW[2] - mass * r[0] * r[2]; ci[5] = IW[5] - mass * r[1] * r[2];
    ci[6] = mass * r[0]; ci[7] = mass * r[1]; ci[8] = mass * r[2]; ci[9] = mass;
  }
  __syncthreads();
  if (lane < nbody) {  // the composite inertia of the subtree
    float s[10];
    for (int i = 0; i < 10; i++) s[i] = 0.f;
    for (int k = lane; k < send; k++)
      for (int i = 0; i < 10; i++) s[i] += cinert[k][i];
    for (int i = 0; i < 10; i++) crb[lane][i] = s[i];
  }
  __syncthreads();

  // ---- lane = dof: cdof about c0 and the composite's momentum f = crb[body] cdof
  const bool isd = lane < nv;
  const DofRec dr = ldrec(&m->drec[isd ? lane : 0]);
  if (lane < NV) {
    float c6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, f[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (isd) {
      float ax[3], an[3];
      const int kind = dyn_dof_axis(dr, lane, xpos, xquat, dax, danc, nbody, ax, an);
      const int root = max(0, min(dr.rootid, nbody - 1)), b = max(0, min(dr.bodyid, nbody - 1));
      if (kind == 1) {
        for (int i = 0; i < 3; i++) c6[3 + i] = ax[i];
      } else {
        const float off[3] = {scom[root][0] - an[0], scom[root][1] - an[1], scom[root][2] - an[2]};
        for (int i = 0; i < 3; i++) c6[i] = ax[i];
        add_cross(c6 + 3, ax, off);
      }
      inert_vec(f, crb[b], c6);
    }
    for (int i = 0; i < 6; i++) { cdof[lane][i] = c6[i]; fd[lane][i] = f[i]; }
  }
  __syncthreads();

  // ---- lane = row: M[i][j] = cdof_anc . f_desc along the chain, armature on the diagonal, identity past nv
  const int row = lane & 31;  // (the upper half repeats the lower one's rows and stores nothing)
  float a[NV];
  {
    const bool isr = row < nv;
    const DofRec rr = ldrec(&m->drec[isr ? row : 0]);
    const uint32_t ancm = isr ? rr.ancmask : 0u, descm = isr ? m->dof_descmask[row] : 0u;
#pragma unroll
    for (int j = 0; j < NV; j++) {
      const bool up = (ancm >> j) & 1u, dn = (descm >> j) & 1u;
      float v = j == row ? 1.f : 0.f;
      if (isr && j < nv) {
        v = 0.f;
        if (up || dn) {
          const int lo = up ? j : row, hi = up ? row : j;
          v = dyn_dot6(cdof[lo], fd[hi]);
          if (j == row) v += rr.armature;
        }
      }
      a[j] = v;
    }
  }
  if (A.full_m) {
    if (lane < NV) {
#pragma unroll
      for (int j = 0; j < NV; j++) Ms[lane * LD + j] = a[j];
    }
    __syncthreads();
    float* o = A.full_m + (size_t)env * nv * nv;
    int r = lane / max(nv, 1), c = lane - r * nv;
    for (int i = lane; i < nv * nv; i += 64) {
      o[i] = Ms[r * LD + c];
      c += 64;
      while (c >= nv) { c -= nv; r++; }
    }
    __syncthreads();
  }
  if (A.mul_m) {
    for (int k = 0; k < nvec; k++) {
      const size_t o = ((size_t)env * nvec + k) * nv;
      const float v = isd ? A.vec[o + lane] : 0.f;
      float y = 0.f;
#pragma unroll
      for (int j = 0; j < NV; j++) y = fmaf(a[j], rdlane(v, j), y);
      if (isd) A.mul_m[o + lane] = y;
    }
  }
  if (!A.solve_m) return;

  // ---- M = L L': rows in registers, column k's broadcasts by readlane; invd = 1 / L[i][i]
  float invd = 1.f;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    const float piv = rdlane(a[k], k);
    const float lkk = sqrtf(piv), inv = 1.f / lkk;
    a[k] = (row == k) ? lkk : a[k] * inv;
    invd = (row == k) ? inv : invd;
#pragma unroll
    for (int j = k + 1; j < NV; j++) a[j] = fmaf(-a[k], rdlane(a[k], j), a[j]);
  }
  // the columns of L: c[k] = L[k][row]
  float c[NV];
  if (lane < NV) {
#pragma unroll
    for (int j = 0; j < NV; j++) Ms[lane * LD + j] = a[j];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) c[k] = Ms[k * LD + row];
  for (int kv = 0; kv < nvec; kv++) {
    const size_t o = ((size_t)env * nvec + kv) * nv;
    float x = isd ? A.vec[o + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < NV; k++) {  // L y = v
      const float yk = rdlane(x, k) * rdlane(invd, k);
      x = (row == k) ? yk : (row > k ? fmaf(-a[k], yk, x) : x);
    }
#pragma unroll
    for (int k = NV - 1; k >= 0; k--) {  // L' z = y
      const float zk = rdlane(x, k) * rdlane(invd, k);
      x = (row == k) ? zk : (row < k ? fmaf(-c[k], zk, x) : x);
    }
    if (isd) A.solve_m[o + lane] = x;
  }
}

}  // namespace mjl
