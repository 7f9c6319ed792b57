// Step linearization (mjl_step_jacobian): the transition matrices A = dx'/dx and B = dx'/du of one mjl_step at
// the batch's current state, as include/mjx355.h defines them (mjd_transitionFD's tangent layout, or
// jax.jacobian(mjx.step)'s raw one).
//
// One wave per (env, row group). The wave runs the step's forward once, exactly as vjp_kernel<D, false, 0> runs it
// in implicit mode (load_step_state, smooth_forward, build_rows into the block's global slab, solver, sensors,
// solver_hessian, the factor of Hc, integrate), and then the reverse passes of adjoint.hip once per output row of
// its group, seeded with that row's one-hot (raw) or tangent-basis cotangent formed in LDS.
//
// What persists between rows, and what is zeroed (DESIGN.md "Linearization" has the reading behind it):
//   * the implicit-mode reverse passes write no field of the forward workspace W: they read it;
//   * of the adjoint workspace they read qpos0, qvel0, Lc, invdc and ap (forward values, kept) and accumulate
//     (+=) into the cotangent fields and Mb: those, with the scratch fields between them (lp .. Mb, one
//     contiguous range of WSA), are zeroed before each row;
//   * in the block's global slab the constraint rows are read only; the adjoint scratch behind them (alpha,
//     gamma, posbar per row, the per-contact records) is assigned for every live row / contact before it is
//     read, so it needs nothing between rows.
// So nothing is restored and nothing is snapshotted: the forward state stays resident in LDS.
//
// Tangent layout: the output-side map (mj_differentiatePos, linearised at the post-step quaternion q'0 that
// integrate() left in W->qpos) enters as the seed; the input-side map (mj_integratePos, linearised at the
// pre-step quaternion) contracts the qpos cotangent to nv entries before the store.
// Included by capi.hip after adjoint.hip.
#pragma once

namespace mjl {

struct LinArgs {
  const float* ctrl;   // [nenv, nu]
  const float* mask;   // [nenv] or null
  float* A;            // tangent [nenv, 2nv, 2nv], raw [nenv, nq+nv, nq+nv]; or null
  float* B;            // tangent [nenv, 2nv, nu], raw [nenv, nq+nv, nu]; or null
  float* scratch;      // per block (env * groups + group): row slab, then the adjoint scratch
  int scratch_stride, row_floats;
  int groups;          // row groups per env
  int tangent;
};

// d (q (x) (0, e_k))_j / d e_k = d (conj(q) (x) p)_{1+k} / d p_j: entry (k, j) of the 3 x 4 matrix both tangent maps
// of a free joint's quaternion are built from (input: 1/2 of it at the pre-step q; output: 2 x at q'0)
INL float quat_tangent(int k, int j, float w, float x, float y, float z) {
  if (k == 0) return j == 0 ? -x : (j == 1 ? w : (j == 2 ? z : -y));
  if (k == 1) return j == 0 ? -y : (j == 1 ? -z : (j == 2 ? w : x));
  return j == 0 ? -z : (j == 1 ? y : (j == 2 ? -x : w));
}

template <class D> __global__ __launch_bounds__(64, 1) void linearize_kernel(KParams P, LinArgs L) {
  typedef WSA<D> AT;
  typedef WS<D> WT;
  __shared__ WT Ws;
  __shared__ AT As;
  __shared__ float aux_s[MJL_AUX_DIM + 3];
  LDSA WT* W = (LDSA WT*)&Ws;
  LDSA AT* A = (LDSA AT*)&As;
  LDSA float* aux = (LDSA float*)aux_s;
  static_assert(MJL_MAXQ <= 3 * D::LD, "the qpos' seed is staged in WSA::uv (unused by the implicit mode)");
  // the fields the reverse passes accumulate into or use as scratch: one contiguous range of WSA
  constexpr int Z0 = (int)(offsetof(AT, lp) / 4), Z1 = (int)(offsetof(AT, qfcb) / 4);
  static_assert(offsetof(AT, lp) > offsetof(AT, ap) && offsetof(AT, qfcb) > offsetof(AT, Mb) &&
                    offsetof(AT, lp) % 4 == 0 && offsetof(AT, qfcb) % 4 == 0,
                "lp .. Mb lie between the kept forward values and the unrolled mode's fields");
  MP m = (MP)P.m;
  const int lane = threadIdx.x;
  const int env = (int)blockIdx.x / L.groups, grp = (int)blockIdx.x - env * L.groups;
  if (env >= P.nenv) return;
  if (L.mask && !(L.mask[env] > 0.5f)) return;
  const int nq = m->nq, nv = m->nv, nu = m->nu;
  const int nin = L.tangent ? nv : nq;  // width of the position block, rows and columns
  const int nrow = nin + nv;
  const int per = (nrow + L.groups - 1) / L.groups;
  const int r0 = grp * per, r1 = min(r0 + per, nrow);
  if (r0 >= r1) return;
  float* scr_blk = L.scratch + (size_t)blockIdx.x * (size_t)L.scratch_stride;
  GLBA float* scr_adj = (GLBA float*)(scr_blk + L.row_floats);
  {
    LDSA float* a = (LDSA float*)A;
    for (int i = lane; i < (int)(sizeof(AT) / 4); i += 64) a[i] = 0.f;
    zero_ld_vectors<D>(W, lane);
  }
  SYNC();
  Rows<true> R = global_rows<D>(scr_blk, P.gmax_efc, P.gmax_con);
  {
    const LaneState s0 = load_step_state<D, false, false>(m, P.s, P.env, L.ctrl, W, aux, env, lane);
    if (lane < nq) A->qpos0[lane] = s0.q;
    if (lane < nv) A->qvel0[lane] = s0.v;
  }
  SYNC();
  // ---- forward, once (vjp_kernel's recompute, implicit mode)
  smooth_forward<D, false, false, false>(m, W, lane, kin_prefetch(m, lane));
  SYNC();
  build_rows<D, true>(m, W, R, lane);
  solver<D, true>(m, W, R, lane);
  sensors<D, true>(m, W, R, lane);
  solver_hessian<D, true>(m, W, R, lane);  // Hc at the converged active set
  chol_factor_solve<D>(W->H, A->Lc, A->invdc, nv, W->frc_smooth, lane);
  SYNC();
  integrate<D, false>(m, W, lane, A->ap);
  const AdjMats<const LDSA float*> mats{W->M, W->H, W->invd, A->Lc, A->invdc, nullptr};
  LDSA float* seed = (LDSA float*)&A->uv[0][0];
  const float* seed_g = (const float*)&As.uv[0][0];  // adj_integrate reads the qpos' cotangent through a flat pointer
  // this lane's column of the position block (tangent: dof `lane`, raw: qpos entry `lane`)
  const DofRec cdr = ldrec(&m->drec[lane < nv ? lane : 0]);
  const int cqa = m->jrec[cdr.jntid].qadr;
  // ---- reverse, once per row of the group (row, and every bound below, is wave-uniform)
  for (int row = r0; row < r1; row++) {
    {
      LDSA float* a = (LDSA float*)A;
      for (int i = Z0 + lane; i < Z1; i += 64) a[i] = 0.f;
    }
    SYNC();
    // the row's cotangent of (qpos', qvel')
    float sq = 0.f;
    if (row < nin) {
      if (!L.tangent) {
        sq = lane == row ? 1.f : 0.f;
      } else {
        const int kf = m->drec[row].kfree, qa = m->jrec[m->drec[row].jntid].qadr;
        if (kf < 3) {  // hinge, or a free joint's position: the coordinate itself
          sq = lane == qa + max(kf, 0) ? 1.f : 0.f;
        } else {       // delta'_k = 2 (conj(q'0) (x) dq')_{1+k}
          const int j = lane - (qa + 3);
          if (j >= 0 && j < 4)
            sq = 2.f * quat_tangent(kf - 3, j, W->qpos[qa + 3], W->qpos[qa + 4], W->qpos[qa + 5], W->qpos[qa + 6]);
        }
      }
    }
    if (lane < MJL_MAXQ) seed[lane] = lane < nq ? sq : 0.f;
    if (lane < nv) A->vtmp[lane] = (row >= nin && lane == row - nin) ? 1.f : 0.f;
    SYNC();
    adj_integrate<D>(m, W, A, mats, seed_g, false, lane);
    SYNC();
    adj_solver_rows<D>(m, W, A, mats, R, scr_adj, P.gmax_efc, lane);
    adj_contact_jac<D>(m, W, A, R, scr_adj, P.gmax_efc, (GLBA const float*)nullptr, lane);
    adj_collision<D>(m, W, A, R, scr_adj, P.gmax_efc, lane);
    adj_geom_frames<D>(m, A, lane);
    adj_forces<D>(m, W, A, lane);  // ctrl-bar is final here: with A null the row ends
    if (L.B && lane < nu) L.B[((size_t)env * nrow + row) * nu + lane] = A->ctrlb[lane];
    if (L.A) {
      adj_rne<D>(m, W, A, lane);
      adj_mass<D>(m, W, A, mats, false, lane);
      adj_crb<D>(m, A, lane);
      adj_cinert<D>(m, W, A, lane);
      adj_cdof<D>(m, W, A, lane);
      adj_kinematics<D>(m, W, A, lane);
      float* out = L.A + ((size_t)env * nrow + row) * nrow;
      if (!L.tangent) {
        if (lane < nq) out[lane] = A->qposb[lane];
      } else if (lane < nv) {
        const int kf = cdr.kfree;
        float o;
        if (kf < 3) {
          o = A->qposb[cqa + max(kf, 0)];
        } else {  // dq = 1/2 q (x) (0, delta)
          const float w = A->qpos0[cqa + 3], x = A->qpos0[cqa + 4], y = A->qpos0[cqa + 5], z = A->qpos0[cqa + 6];
          o = 0.f;
          for (int j = 0; j < 4; j++) o += quat_tangent(kf - 3, j, w, x, y, z) * A->qposb[cqa + 3 + j];
          o *= 0.5f;
        }
        out[lane] = o;
      }
      if (lane < nv) out[nin + lane] = A->qvelb[lane];
    }
    SYNC();  // the row's reads of the cotangents, before the next row zeroes them
  }
}

}  // namespace mjl
