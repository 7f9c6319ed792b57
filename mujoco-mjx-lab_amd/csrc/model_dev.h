// Device-side model constants (float32) and kernel parameter block.
// Built on the host from mjlModelDesc (include/mjx355.h) by model_build (model_host.h); lives in device
// global memory, read through the scalar/vector caches (a few KB, shared by every env).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/mjx355.h"

namespace mjl {

// Packed per-lane records (16-byte rows -> one b128 load each): a phase loads the records of
// its lane once, up front, instead of walking dependent index chains inside its level loops.
struct alignas(16) BodyRec {
  int parent, level, jntadr, jntnum;
  int dofadr, dofnum, subtree_end, rootid;
  int isfree, qadr, pad0, pad1;  // isfree: the body's only joint is free (qadr: its qpos address)
  float pos[3], mass;
  float quat[4];
  float ipos[3], pad2;
  float inertia[6], pad3[2];  // body_inertia (local principal frame: xx yy zz xy xz yz)
};
// the first three hinges of a body (kinematics' local transform), by body: one load with the body's
// own record instead of a second load through jntadr
struct alignas(16) HingeRec {
  float pos[3], pad0;
  float axis[3], pad1;
};
// geom (index < 32) / site (index 32 + s) frame constants, by lane: body, local pos, local z axis
// (geoms, mat[0..2]) or local rotation (sites)
constexpr int kSiteLane = 32;  // ModelF::frec[kSiteLane + s] is site s; the geoms take the lanes below it
static_assert(MJL_MAXGEOM <= kSiteLane && kSiteLane + MJL_MAXSITE <= 64, "geom and site frames share one 64-lane table");
struct alignas(16) FrameRec {
  int body, pad0, pad1, pad2;
  float pos[3], pad3;
  float mat[9], pad4[3];
};
struct alignas(16) JntRec {  // hinge joints (local frame of the body)
  float pos[3], qpos0;
  float axis[3];
  int qadr;
  int body, parent, isfree, dofadr;
};
struct alignas(16) DofRec {
  int bodyid, jntid, rootid, kfree;  // kfree: index 0..5 inside a free joint, -1 otherwise
  uint32_t ancmask;                  // bit j set <=> dof j is this dof or one of its ancestors
  int qadr_spring;                   // qpos address of a hinge spring, -1 when none
  float damping, armature;
  float stiffness, qpos_spring, invweight0, pad;
};
struct alignas(16) PairRec {
  int g1, g2, kind, condim;
  float r1, h1, r2, h2;  // geom_size[:, 0:2] of both geoms
  float includemargin, mu, invweight, pad;
  uint32_t mask1, mask2;  // body_dofmask of both bodies
  int b1, b2;
};
// a limit-row candidate: lane = joint (limited hinge) or lane = tendon (limited tendon); everything
// the row needs, including its impedance parameters, in one record
struct alignas(16) LimRec {
  int on, qadr, dofadr, pad;  // on: the joint / tendon is a limit-row candidate
  float lo, hi, margin, invweight;
  float solref[2], solimp[5], pad1;
};

// a general actuator (MJL_ACT_GENERAL; a motor of a model that has one is written as gain 1, no bias, no limit):
// force = gain * clip(ctrl) + b0 + b1 * gear * qpos[qadr] + b2 * gear * qvel[dof], clipped to [flo, fhi] when
// flim; gear, the dof and the ctrl range stay in the flat actuator_* members (one home: a per-env gear is
// followed by length, velocity, moment and the integrator's gear^2 * b2 without any derived copy)
struct alignas(16) ActRec {
  float gain, b0, b1, b2;
  float flo, fhi;
  int flim, qadr;
};

// ModelF holds exactly what a kernel reads. Host staging does not belong here: a value the kernels take
// only through a record is written into the record straight from mjlModelDesc (model_host.h) and has no
// flat array. A member is added here together with the kernel read that needs it, and removed with it.
//
// Constants that still have two homes, and who reads which (moving a read from one home to the other
// changes a kernel's loads: a change of its own, with a measurement):
//   body_subtree_end   flat: subtree centres of mass over the roots (step kinematics), the renderer's
//                      tracking camera; BodyRec.subtree_end: the subtree sums of CRB and RNE
//   jnt_qposadr        flat: the limit rows' position cotangent (adjoint, by row id); JntRec.qadr /
//                      BodyRec.qadr: kinematics, integration and their reverse passes, the renderer;
//                      LimRec.qadr: the limit rows (step); DofRec.qadr_spring: passive forces
//   jnt_range, jnt_solref, jnt_solimp, tendon_range, tendon_solref, tendon_solimp
//                      flat: the adjoint of the constraint rows (by row id); LimRec (jlim / tlim): the
//                      limit rows of the step
//   dof_damping        flat: the integrator's damping term (step); DofRec.damping: passive forces and
//                      their adjoint
//   qpos0              flat: reset (whole vector); JntRec.qpos0: hinge angles in kinematics, its
//                      reverse pass and the renderer
//   qpos_spring        flat: whole vector, kept beside qpos0; DofRec.qpos_spring: passive forces
//   geom_size          flat: the renderer's primitives; PairRec.r1/h1/r2/h2: collision and its adjoint
//   site_bodyid        flat: touch sensors (by sensor_objid); FrameRec.body (lanes 32 + s): site frames
struct ModelF {
  int nq, nv, nu, nbody, njnt, ngeom, nsite, ntendon, npair, nsensor, nsensordata;
  int iterations, ls_iterations, solver, integrator, eulerdamp, maxlevel, any_damping;
  int nroot, root[MJL_MAXBODY];  // kinematic roots: bodies whose parent is the world
  float timestep, gravity[3], tolerance, ls_tolerance, scale;

  int body_subtree_end[MJL_MAXBODY];
  // tree walks of the reverse passes as bit loops (no record loads in the loop): ancestors-or-self
  // (world excluded), children, children without a free joint, joints whose world anchor / axis
  // cotangents gather into b (b's free joint, hinges of b's children); the float sum of the masses
  // of root r's subtree in body order
  uint32_t body_ancmask[MJL_MAXBODY], body_childmask[MJL_MAXBODY], body_childmask_nf[MJL_MAXBODY];
  uint32_t body_jgather[MJL_MAXBODY];
  uint32_t dof_descmask[MJL_MAXV];  // bit i set <=> dof i is this dof or one of its descendants
  uint32_t body_geommask[MJL_MAXBODY];  // bit g set <=> geom g belongs to body b
  float body_rootmass[MJL_MAXBODY];

  int jnt_qposadr[MJL_MAXJNT];
  float jnt_range[MJL_MAXJNT][2], jnt_solref[MJL_MAXJNT][2], jnt_solimp[MJL_MAXJNT][5];

  float dof_damping[MJL_MAXV];
  float qpos0[MJL_MAXQ], qpos_spring[MJL_MAXQ];

  int geom_type[MJL_MAXGEOM];
  float geom_size[MJL_MAXGEOM][3];

  float pair_solref[MJL_MAXPAIR][2], pair_solimp[MJL_MAXPAIR][5];

  int site_bodyid[MJL_MAXSITE];
  float site_size[MJL_MAXSITE][3];

  int actuator_dof[MJL_MAXU], actuator_ctrllimited[MJL_MAXU];
  float actuator_gear[MJL_MAXU], actuator_ctrlrange[MJL_MAXU][2];

  int tendon_num[MJL_MAXTENDON], tendon_qadr[MJL_MAXTENDON][MJL_MAXTENWRAP];
  int tendon_dof[MJL_MAXTENDON][MJL_MAXTENWRAP];
  float tendon_coef[MJL_MAXTENDON][MJL_MAXTENWRAP], tendon_range[MJL_MAXTENDON][2];
  float tendon_solref[MJL_MAXTENDON][2], tendon_solimp[MJL_MAXTENDON][5];

  int sensor_objid[MJL_MAXSENSOR], sensor_adr[MJL_MAXSENSOR];

  BodyRec brec[MJL_MAXBODY];
  JntRec jrec[MJL_MAXJNT];
  DofRec drec[MJL_MAXV];
  PairRec prec[MJL_MAXPAIR];
  LimRec jlim[MJL_MAXJNT], tlim[MJL_MAXTENDON];
  HingeRec bhinge[MJL_MAXBODY][3];
  FrameRec frec[64];

  // General actuators, after everything a motor-only model has: up to here the block of a model without one
  // is laid out and filled as it always was, and the rest of it is zero.
  //   act_general  some actuator is MJL_ACT_GENERAL: the actuation phase takes arec (a scalar branch)
  //   act_b2       some arec[u].b2 != 0: under implicitfast the integrator's matrix gets
  //                -dt * sum_u gear_u^2 b2_u on the diagonal, also when every dof_damping is 0
  ActRec arec[MJL_MAXU];
  int act_general, act_b2, act_pad[2];
};

// The size MJL_OPT_PER_ENV_MODEL allocates per env is stated in include/mjx355.h, README.md, INTEGRATION.md and
// DESIGN.md ("Per-env model parameters"): a change of ModelF changes those figures with this one.
static_assert(offsetof(ModelF, arec) == 45936, "the motor-only part of the block keeps its layout");
static_assert(sizeof(ModelF) == 46976, "sizeof(ModelF) is documented: update the figures named above");

// The readout table of mjl_sensors (sensor_kernels.hip): a small block of its own beside the model block, so
// ModelF and the per-env model blocks keep their size. Built by sensor_tab_build (model_host.h).
struct SensorTab {
  int n, ndata, stages, pad;  // stages: the MJL_SENS_STAGE_* bits some entry has
  int type[MJL_MAXRSENSOR], objtype[MJL_MAXRSENSOR], objid[MJL_MAXRSENSOR];
  int adr[MJL_MAXRSENSOR], dim[MJL_MAXRSENSOR], stage[MJL_MAXRSENSOR];
  float site_quat[MJL_MAXSITE][4];
};
// What mjl_body_data (body_kernels.hip) reads beside the model block: body_iquat, the principal axes of the
// descriptor's body-frame inertia tensor (the descriptor and ModelF hold the tensor, not MuJoCo's principal
// moments + quaternion). Read for the ximat output only. Built by body_tab_build (model_host.h).
struct BodyTab {
  float iquat[MJL_MAXBODY][4];
};
// What mjl_jac (dyn_kernels.hip) reads beside the model block: bit k of body_dofmask[b] set <=> dof k moves body b
// (the dofs of b and of its ancestors), the columns of b's Jacobian that are not zero. Row 0 is 0. Built by
// dyn_tab_build (model_host.h).
struct DynTab {
  uint32_t body_dofmask[MJL_MAXBODY];
};
// dim and stage of a sensor type (MJL_SENS_*)
constexpr int sensor_type_dim(int type) {
  return type == MJL_SENS_FRAMEQUAT ? 4
         : (type == MJL_SENS_TOUCH || type == MJL_SENS_JOINTPOS || type == MJL_SENS_JOINTVEL ||
            type >= MJL_SENS_ACTUATORFRC) ? 1 : 3;
}
constexpr int sensor_type_stage(int type) {
  return (type == MJL_SENS_TOUCH || type >= MJL_SENS_ACCELEROMETER) ? MJL_SENS_STAGE_ACC
         : (type == MJL_SENS_JOINTVEL || (type >= MJL_SENS_GYRO && type <= MJL_SENS_FRAMEANGVEL)) ? MJL_SENS_STAGE_VEL
         : MJL_SENS_STAGE_POS;
}

// MODE_APPLIED: a flag on MODE_FORWARD / MODE_STEP / MODE_ENV_STEP in step_kernel's template argument, the
// instantiations that read the applied forces (KParams::qfrc_applied / xfrc_applied)
// MODE_PER_ENV: a flag beside it, on those three and on MODE_ENV_RESET: env e reads the model block
// KParams::m_env[e] (MJL_OPT_PER_ENV_MODEL) instead of KParams::m
enum Mode { MODE_FORWARD = 0, MODE_STEP = 1, MODE_SPEEDTEST = 2, MODE_ENV_STEP = 3, MODE_ENV_RESET = 4,
            MODE_APPLIED = 8, MODE_PER_ENV = 16 };

// What the per-env model builder (model_params_kernel) needs and ModelF does not hold: built on the host by
// model_param_stage (model_host.h), one per batch on the device.
struct ParamStage {
  double impratio;
  double tran[MJL_MAXPAIR];  // body_invweight0[b1][0] + body_invweight0[b2][0] of the pair's bodies
};

// per-env state rows, [nenv, dim] each
struct StateBuf {
  float *qpos, *qvel, *qacc_warmstart, *time, *ctrl, *aux;
  // derived (outputs of the last forward pass)
  float *qacc, *xpos, *xquat, *qfrc_actuator, *sensordata, *stats;
  float *qfrc_bias, *qfrc_passive, *qfrc_constraint, *qacc_smooth;
};
// the member behind each MJL_FIELD_* index, in index order (host side: the kernels name the members)
inline constexpr float* StateBuf::*kStateField[] = {
    &StateBuf::qpos,           &StateBuf::qvel,         &StateBuf::qacc_warmstart,  &StateBuf::time,
    &StateBuf::ctrl,           &StateBuf::qacc,         &StateBuf::xpos,            &StateBuf::xquat,
    &StateBuf::qfrc_actuator,  &StateBuf::sensordata,   &StateBuf::aux,             &StateBuf::stats,
    &StateBuf::qfrc_bias,      &StateBuf::qfrc_passive, &StateBuf::qfrc_constraint, &StateBuf::qacc_smooth};
static_assert(sizeof(kStateField) / sizeof(kStateField[0]) == MJL_NFIELD && sizeof(StateBuf) == MJL_NFIELD * sizeof(float*),
              "one StateBuf member per field");
static_assert(MJL_FIELD_QPOS == 0 && MJL_FIELD_QVEL == 1 && MJL_FIELD_QACC_WARMSTART == 2 && MJL_FIELD_TIME == 3 &&
                  MJL_FIELD_CTRL == 4 && MJL_FIELD_QACC == 5 && MJL_FIELD_XPOS == 6 && MJL_FIELD_XQUAT == 7 &&
                  MJL_FIELD_QFRC_ACTUATOR == 8 && MJL_FIELD_SENSORDATA == 9 && MJL_FIELD_AUX == 10 &&
                  MJL_FIELD_STATS == 11 && MJL_FIELD_QFRC_BIAS == 12 && MJL_FIELD_QFRC_PASSIVE == 13 &&
                  MJL_FIELD_QFRC_CONSTRAINT == 14 && MJL_FIELD_QACC_SMOOTH == 15,
              "kStateField is in MJL_FIELD_* order");

struct KParams {
  const ModelF* m;
  const mjlEnvConfig* env;
  StateBuf s;
  int nenv;
  int store_derived;
  int force_global_rows;  // test hook: always use the global-scratch row storage
  int auto_reset;
  const float* in_ctrl;   // [nenv, nu] or null
  const float* mask;      // [nenv] or null
  const float* noise;     // [nenv, nq-7+nv+2] or null
  const float* vel;       // speed test input
  float* out_speed;       // speed test output
  float *obs, *rew, *term, *trunc;
  float* scratch;         // global overflow rows, [nenv, scratch_stride]
  int scratch_stride;    // floats per env
  int gmax_efc, gmax_con; // row / contact capacity of one scratch slab
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
  const unsigned long long* ctr_base;  // device counter base added to (ctr_hi, ctr_lo), or null
  const uint32_t* keys;                // per-env jax.random reset keys [nenv, 2], or null
  int key_mode;                        // MJL_RNG_* of `keys`
  // reset pool (mjl_env_fill_reset_pool): slot j of env e is row j * nenv + e of `rs` / rs_obs
  StateBuf rs;
  float* rs_obs;    // [slots * nenv, obs_dim]
  int* pool_ctl;    // [nenv, 2]: next unused slot, filled slots; null = no pool
  const int* pool_n;  // fill: slots to fill (device int, read at execution time)
  int pool_slot;    // fill: the slot this launch draws (-1: not a fill)
  int pool_slots;   // fill: pool capacity (slots per env)
  // applied forces (mjl_batch_attach_applied), read by the MODE_APPLIED instantiations only
  const float* qfrc_applied;  // [nenv, nv] or null
  const float* xfrc_applied;  // [nenv, nbody, 6] world-frame (force, torque) at xipos, or null
  // per-env model blocks (MJL_OPT_PER_ENV_MODEL), read by the MODE_PER_ENV instantiations only
  const ModelF* m_env;  // [nenv] or null
};

}  // namespace mjl
