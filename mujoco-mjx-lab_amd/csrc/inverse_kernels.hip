// Inverse dynamics (mjl_inverse): the generalized force that gives the batch's state a prescribed acceleration,
// contacts and limits included, as include/mjx355.h defines it (mj_inverse / mjx.inverse).
//
// One kernel, one wavefront per env, on the step kernel's workspace WS<D> and its phases, called as mjl_forward's
// launch calls them (each is inlined here, so no instantiation of the step kernel shares code with this one):
//   1. qpos, qvel and the acceleration a into LDS (ctrl = 0: the actuator force takes no part in the result).
//   2. smooth_forward: kinematics, composite inertia and M, bias and passive forces, the factor of M into H.
//   3. MJL_INV_DISCRETE, under integrate()'s condition: k = dof_damping - (implicitfast) sum_u gear_u^2 b2_u,
//      a_c = a + timestep M^-1 (k o a) by the two substitutions on the factor in H. Otherwise a_c = a.
//   4. build_rows into the LDS rows; when they overflow or the launch forces it, into the env's global slab.
//   5. One pass over the rows (lane = row): jar = J a_c - aref, force = -D jar where jar < 0, else 0; then
//      qfrc_constraint = J' force (lane & 31 = dof, the two halves of the wave on alternate rows).
//   6. qfrc_inverse = M a_c + qfrc_bias - qfrc_passive - qfrc_constraint (lane = dof).
// No solver, no sensors phase, nothing of the batch written: the rows (LDS or the env's slab of the batch's row
// scratch) are the only workspace.
// Included by capi.hip after step_kernels.hip.
#pragma once

namespace mjl {

struct InvArgs {
  const ModelF* m;
  const ModelF* m_env;   // [nenv] per-env blocks (MJL_OPT_PER_ENV_MODEL), or null
  const float *qpos, *qvel;
  const float* qacc;     // [nenv, nv]
  const float* mask;     // [nenv] or null
  float* qfrc_inverse;   // [nenv, nv]
  float* qfrc_constraint;  // [nenv, nv] or null
  float* scratch;        // the batch's global row slabs, [nenv, scratch_stride]
  int scratch_stride, gmax_efc, gmax_con;
  int nenv, flags, force_global_rows;
};

// force = -D (J a_c - aref) on the rows with a negative residual, then frc_con = J' force (solver_update's sum)
template <class D, bool G> INL void inverse_rows(MP m, LDSA WS<D>* W, Rows<G> R, int lane) {
  constexpr int LD = D::LD;
  const int nv = m->nv, nefc = uni_int(W->nefc);
  for (int r = lane; r < nefc; r += 64) {
    const float jar = jrow<D>(R.J, W->qacc, r) - R.aref[r];
    R.jar[r] = jar;
    R.force[r] = jar < 0.f ? -R.D[r] * jar : 0.f;
  }
  SYNC();  // force is read across lanes below
  const int d = lane & 31, h = lane >> 5;
  float s = 0.f;
  if (d < nv) {
    int r = h;
    for (; r + 6 < nefc; r += 8)  // 4 rows per trip: the loads issue together
      s += R.J[r * LD + d] * R.force[r] + R.J[(r + 2) * LD + d] * R.force[r + 2] +
           R.J[(r + 4) * LD + d] * R.force[r + 4] + R.J[(r + 6) * LD + d] * R.force[r + 6];
    for (; r < nefc; r += 2) s += R.J[r * LD + d] * R.force[r];
  }
  s += __shfl_xor(s, 32);
  if (lane < nv) W->frc_con[lane] = s;
}

template <class D> __global__ __launch_bounds__(64, MJL_MINWAVES) void inverse_kernel(InvArgs A) {
  __shared__ WS<D> Ws;
  LDSA WS<D>* W = (LDSA WS<D>*)&Ws;
  const int env = block_env(), lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  zero_ld_vectors<D>(W, lane);
  SYNC();
  const KinPre kp = kin_prefetch(m, lane);  // issued before the state loads: the latencies overlap
  const int iq = lane < nq ? lane : max(nq - 1, 0), iv = lane < nv ? lane : max(nv - 1, 0);
  const float q = nq > 0 ? A.qpos[(size_t)env * nq + iq] : 0.f;
  const float v = nv > 0 ? A.qvel[(size_t)env * nv + iv] : 0.f;
  const float a = (nv > 0 && lane < nv) ? A.qacc[(size_t)env * nv + iv] : 0.f;
  if (lane < nq) W->qpos[lane] = q;
  if (lane < nv) W->qvel[lane] = v;
  if (lane < nu) W->ctrl[lane] = 0.f;
  SYNC();
  smooth_forward<D, false>(m, W, lane, kp);

  // ---- the acceleration the rows and M see: a, or the continuous-time one behind a finite difference
  float ac = a;
  if (A.flags & MJL_INV_DISCRETE) {
    const float dt = m->timestep;
    float k = m->dof_damping[(lane & 31) < nv ? (lane & 31) : 0];
    bool damp = (m->integrator == MJL_INT_IMPLICITFAST || m->eulerdamp) && m->any_damping;
    if (m->act_b2 != 0 && m->integrator == MJL_INT_IMPLICITFAST) {  // integrate()'s diagonal
      for (int u = 0; u < nu; u++) {
        const float g = m->actuator_gear[u];
        if (m->actuator_dof[u] == (lane & 31)) k -= g * g * m->arec[u].b2;
      }
      damp = true;
    }
    if (damp) {
      SYNC();  // the factor of M in H / invd
      const float x = chol_solve<D>(W->H, W->invd, lane < nv ? k * a : 0.f, lane);
      ac = fmaf(dt, x, a);
    }
  }
  if (lane < nv) W->qacc[lane] = ac;  // (build_rows' barriers come before the rows read it)

  bool ok = false;
  if (!A.force_global_rows) ok = build_rows<D, false>(m, W, lds_rows<D>(W), lane);
  if (ok) {
    inverse_rows<D, false>(m, W, lds_rows<D>(W), lane);
  } else {  // more rows than fit in LDS (or forced): this env's slab of global scratch
    Rows<true> R = global_rows<D>(A.scratch + (size_t)env * (size_t)A.scratch_stride, A.gmax_efc, A.gmax_con);
    ok = build_rows<D, true>(m, W, R, lane);
    if (ok) inverse_rows<D, true>(m, W, R, lane);
  }
  SYNC();
  if (lane < nv) {
    const size_t o = (size_t)env * nv + lane;
    const float nan = __int_as_float(0x7fc00000);  // rows past the slab's capacity (the model's own bound): no result
    const float fc = ok ? W->frc_con[lane] : nan;
    A.qfrc_inverse[o] = (mrow<D>(W, W->qacc, lane) + W->frc_bias[lane]) - W->frc_passive[lane] - fc;
    if (A.qfrc_constraint) A.qfrc_constraint[o] = fc;
  }
}

}  // namespace mjl
