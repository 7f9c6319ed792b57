// Sensor readout (mjl_sensors): Data.sensordata of the batch's current state, every sensor of the model's
// readout table (SensorTab, model_dev.h) as MuJoCo defines it (mj_sensorPos / mj_sensorVel / mj_sensorAcc).
//
// A kernel of its own with a workspace of its own (about 5 KB of LDS): nothing of the step kernel's workspace,
// model block or phases is touched, and none of its out-of-line functions is called from here (a second
// caller changes the code the compiler makes for them). One instantiation for any model within the MJL_MAX*
// capacities, one wavefront per env:
//   1. qpos, qvel (and, with the acc stage, the forward pass's qacc) into LDS.
//   2. Tree pass, lane = body, one level at a time from the parent's LDS entry: the body frame (xpos, xquat,
//      MuJoCo's joint order: anchor and axis from the frame before the joint's own rotation) and, by the
//      classical rigid-body recursion along the same chain, the body's angular velocity w and acceleration
//      dw/dt and its origin's linear velocity and acceleration in the world frame. Each hinge moves the
//      reference point to its anchor (fixed in the frames on both sides of the joint) and adds its rate:
//        v_c = v_r + w x d,  a_c = a_r + dw x d + w x (w x d),  d = c - r
//        dw += axis qacc_j + (w x axis) qvel_j,  w += axis qvel_j
//      A free joint gives w = R qvel[3:6], dw = R qacc[3:6] (local angular rates) and v, a = qvel / qacc[0:3].
//   3. Lane = sensor, in trips of 64: the value into the env's LDS row. Touch values, qfrc_actuator and qacc
//      come from the derived store of the forward pass the call ran first, jointlimitfrc from the limit rows
//      (the first rows, emeta = joint id) of the env's global row slab, actuatorfrc from the expression of
//      the step kernel's actuation phase on the env's own model block.
//   4. The row's written slots to out[env], consecutive lanes storing consecutive floats.
// Included by capi.hip after step_kernels.hip (small math, ldrec, uniform_ptr, the slab's array lists).
#pragma once

namespace mjl {

struct SensorArgs {
  const ModelF* m;        // the shared model block
  const ModelF* m_env;    // [nenv] per-env blocks (MJL_OPT_PER_ENV_MODEL), or null
  const SensorTab* tab;
  StateBuf s;
  const float* mask;      // [nenv] or null
  float* scratch;         // the global row slabs (read with the acc stage only)
  int scratch_stride, gmax_efc, gmax_con, LD;
  int nenv, stages;
  float* out;             // [nenv, tab->ndata]
};

// the force and emeta arrays of an env's row slab (the walk of global_rows, the row stride a run-time value)
static INL void slab_force_emeta(float* base_generic, int LD, int nefc_max, const GLBA float*& force,
                                 const GLBA int*& emeta) {
  GLBA float* p = (GLBA float*)base_generic + (size_t)nefc_max * LD;
  const GLBA float* f_force = nullptr;
  const GLBA int* f_emeta = nullptr;
#define MJL_PICK_force(T) f_force = (const GLBA float*)p;
#define MJL_PICK_emeta(T) f_emeta = (const GLBA int*)p;
#define MJL_PICK_D(T)
#define MJL_PICK_aref(T)
#define MJL_PICK_jar(T)
#define MJL_PICK_Jv(T)
#define MJL_PICK_epos(T)
#define MJL_PICK_einvw(T)
#define X(T, f) MJL_PICK_##f(T) p += nefc_max;
  MJL_EFC_ARRAYS(X)
#undef X
#undef MJL_PICK_force
#undef MJL_PICK_emeta
#undef MJL_PICK_D
#undef MJL_PICK_aref
#undef MJL_PICK_jar
#undef MJL_PICK_Jv
#undef MJL_PICK_epos
#undef MJL_PICK_einvw
  force = f_force; emeta = f_emeta;
}

// r += a x b
static INL void add_cross(float* r, const float* a, const float* b) {
  r[0] += a[1] * b[2] - a[2] * b[1];
  r[1] += a[2] * b[0] - a[0] * b[2];
  r[2] += a[0] * b[1] - a[1] * b[0];
}
// the velocity and acceleration of the point r + d of a frame with rates (w, dw): v += w x d, a += dw x d + w x (w x d)
static INL void move_point(float* v, float* a, const float* w, const float* dw, const float* d) {
  float wd[3] = {0.f, 0.f, 0.f};
  add_cross(wd, w, d);
  v[0] += wd[0]; v[1] += wd[1]; v[2] += wd[2];
  add_cross(a, dw, d);
  add_cross(a, w, wd);
}

__global__ __launch_bounds__(64) void sensors_kernel(SensorArgs A) {
  __shared__ float qpos[MJL_MAXQ], qvel[MJL_MAXV], qacc[MJL_MAXV];
  __shared__ float xpos[MJL_MAXBODY][3], xquat[MJL_MAXBODY][4];
  __shared__ float bw[MJL_MAXBODY][3], bdw[MJL_MAXBODY][3], bv[MJL_MAXBODY][3], ba[MJL_MAXBODY][3];
  __shared__ float row[MJL_MAXRSENSORDATA];
  __shared__ int written[MJL_MAXRSENSORDATA];
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= A.nenv) return;
  if (A.mask && !(A.mask[env] > 0.5f)) return;
  const MP m = uniform_ptr((MP)(A.m_env ? A.m_env + env : A.m));
  const SensorTab* T = A.tab;
  const int stages = A.stages;
  const bool acc = (stages & MJL_SENS_STAGE_ACC) != 0;
  const int nq = m->nq, nv = m->nv, nbody = m->nbody, nu = m->nu, maxlevel = m->maxlevel;
  const int ns = min(T->n, MJL_MAXRSENSOR), nd = min(T->ndata, MJL_MAXRSENSORDATA);

  if (lane < nq) qpos[lane] = A.s.qpos[(size_t)env * nq + lane];
  if (lane < nv) {
    qvel[lane] = A.s.qvel[(size_t)env * nv + lane];
    qacc[lane] = acc ? A.s.qacc[(size_t)env * nv + lane] : 0.f;
  }
  for (int i = lane; i < nd; i += 64) written[i] = 0;
  if (lane == 0) {
    xquat[0][0] = 1.f; xquat[0][1] = xquat[0][2] = xquat[0][3] = 0.f;
    for (int i = 0; i < 3; i++) xpos[0][i] = bw[0][i] = bdw[0][i] = bv[0][i] = ba[0][i] = 0.f;
  }
  __syncthreads();

  // ---- tree pass: frames and rates of every body, a level at a time
  const bool isb = lane > 0 && lane < nbody;
  const BodyRec br = ldrec(&m->brec[isb ? lane : 0]);
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

  // ---- the sensors, lane = sensor
  const GLBA float* efc_force = nullptr;
  const GLBA int* efc_meta = nullptr;
  int nefc = 0;
  if (acc) {
    slab_force_emeta(A.scratch + (size_t)env * (size_t)A.scratch_stride, A.LD, A.gmax_efc, efc_force, efc_meta);
    nefc = max(0, min((int)A.s.stats[(size_t)env * 4 + 1], A.gmax_efc));
  }
  for (int s = lane; s < ns; s += 64) {
    if (!(T->stage[s] & stages)) continue;
    const int type = T->type[s], ot = T->objtype[s], id = T->objid[s], adr = T->adr[s], dim = T->dim[s];
    float val[4] = {0.f, 0.f, 0.f, 0.f};
    if (ot == MJL_OBJ_XBODY || ot == MJL_OBJ_SITE) {
      // the frame: origin p, quaternion fq (matrix R), the carrying body's rates moved to p
      int b = id;
      float d[3] = {0.f, 0.f, 0.f}, fq[4] = {xquat[b][0], xquat[b][1], xquat[b][2], xquat[b][3]};
      if (ot == MJL_OBJ_SITE) {
        const FrameRec fr = ldrec(&m->frec[kSiteLane + id]);
        b = fr.body;
        float Rb[9];
        q2m(Rb, xquat[b]);
        mv3(d, Rb, fr.pos);
        qmul(fq, xquat[b], T->site_quat[id]);
      }
      float R[9], p[3], v[3], a[3], w[3];
      q2m(R, fq);
      for (int i = 0; i < 3; i++) { p[i] = xpos[b][i] + d[i]; v[i] = bv[b][i]; a[i] = ba[b][i]; w[i] = bw[b][i]; }
      move_point(v, a, w, bdw[b], d);
      switch (type) {
        case MJL_SENS_FRAMEPOS: for (int i = 0; i < 3; i++) val[i] = p[i]; break;
        case MJL_SENS_FRAMEQUAT: for (int i = 0; i < 4; i++) val[i] = fq[i]; break;
        case MJL_SENS_FRAMEXAXIS: for (int i = 0; i < 3; i++) val[i] = R[3 * i]; break;
        case MJL_SENS_FRAMEYAXIS: for (int i = 0; i < 3; i++) val[i] = R[3 * i + 1]; break;
        case MJL_SENS_FRAMEZAXIS: for (int i = 0; i < 3; i++) val[i] = R[3 * i + 2]; break;
        case MJL_SENS_GYRO: mtv3(val, R, w); break;
        case MJL_SENS_VELOCIMETER: mtv3(val, R, v); break;
        case MJL_SENS_FRAMELINVEL: for (int i = 0; i < 3; i++) val[i] = v[i]; break;
        case MJL_SENS_FRAMEANGVEL: for (int i = 0; i < 3; i++) val[i] = w[i]; break;
        case MJL_SENS_ACCELEROMETER: {
          const float ag[3] = {a[0] - m->gravity[0], a[1] - m->gravity[1], a[2] - m->gravity[2]};
          mtv3(val, R, ag);
          break;
        }
        default: break;
      }
    } else if (ot == MJL_OBJ_JOINT) {
      const JntRec jr = ldrec(&m->jrec[id]);
      switch (type) {
        case MJL_SENS_JOINTPOS: val[0] = qpos[jr.qadr]; break;
        case MJL_SENS_JOINTVEL: val[0] = qvel[jr.dofadr]; break;
        case MJL_SENS_JOINTACTUATORFRC: val[0] = A.s.qfrc_actuator[(size_t)env * nv + jr.dofadr]; break;
        case MJL_SENS_JOINTLIMITFRC:  // the joint limits' rows come first, one per active limit, emeta = the joint
          for (int r = 0; r < nefc && (efc_meta[r] >> 16) == 0; r++)
            if ((efc_meta[r] & 0xffff) == id) val[0] = efc_force[r];
          break;
        default: break;
      }
    } else if (ot == MJL_OBJ_ACTUATOR) {  // the actuation phase's force (velocity_stage), before the gear maps it to the dof
      const int u = min(id, nu - 1), dof = m->actuator_dof[u];
      float c = A.s.ctrl[(size_t)env * nu + u];
      if (m->actuator_ctrllimited[u]) c = fminf(fmaxf(c, m->actuator_ctrlrange[u][0]), m->actuator_ctrlrange[u][1]);
      float force = c;
      if (m->act_general) {
        const ActRec ar = ldrec(&m->arec[u]);
        const float gear = m->actuator_gear[u];
        force = ar.gain * c + (ar.b0 + ar.b1 * (gear * qpos[ar.qadr]) + ar.b2 * (gear * qvel[dof]));
        if (ar.flim) force = fminf(fmaxf(force, ar.flo), ar.fhi);
      }
      val[0] = force;
    } else {  // MJL_OBJ_TOUCH: entry `id` of the touch list, as the forward pass stored it
      val[0] = A.s.sensordata[(size_t)env * m->nsensordata + m->sensor_adr[id]];
    }
    for (int i = 0; i < dim; i++) { row[adr + i] = val[i]; written[adr + i] = 1; }
  }
  __syncthreads();
  float* o = A.out + (size_t)env * (size_t)nd;
  for (int i = lane; i < nd; i += 64)
    if (written[i]) o[i] = row[i];
}

}  // namespace mjl
