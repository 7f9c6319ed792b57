/*
 * mjx355 — MI355X-native batched humanoid physics step (C ABI).
 *
 * This header is the drop-in boundary for the reference's hot path. Each entry
 * point names the reference interface it replaces. The reference calls MJX, a JAX library
 * (mujoco-mjx==3.3.6, requirements.txt:27), from Python:
 *
 *   mujoco.MjModel.from_xml_path + mjx.put_model   src/training_utils.py:80,105
 *                                                  mjx_humanoid_speed_test.py:25,28,44
 *   mjx.make_data + mjx.forward                    src/envs.py:108-113 (single_pipeline_init)
 *   mjx.step                                       src/envs.py:345, mjx_humanoid_speed_test.py:54
 *   v_step = jit(vmap(single_step))                src/envs.py:333-495
 *   v_reset + merge_if_done (auto-reset)           src/envs.py:115-202,494; train_ppo.py:149-161
 *
 * Conventions
 *   - All device buffers are float32, C-contiguous, shape [nenv, dim] (one row per env).
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream). Calls are asynchronous.
 *   - Return value 0 = OK; otherwise an error code and mjl_last_error() holds a message.
 *   - A batch is thread-compatible, not thread-safe. One process per GPU.
 *   - No allocation happens in step/forward/env calls (they can be captured in a hipGraph).
 */
#ifndef MJX355_H_
#define MJX355_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Model descriptor: compiled model constants (float64), the data that mjx.put_model uploads.
 * Filled by the host-side MJCF compiler (mjx_amd/mjcf.py). Capacities below bound the models
 * the kernels accept; larger models are rejected at load time (MJL_ERR_UNSUPPORTED).
 * ------------------------------------------------------------------------------------------- */
#define MJL_MAXBODY 32
#define MJL_MAXJNT 32
#define MJL_MAXQ 48
#define MJL_MAXV 32
#define MJL_MAXGEOM 32
#define MJL_MAXSITE 8
#define MJL_MAXU 32
#define MJL_MAXTENDON 4
#define MJL_MAXTENWRAP 4
#define MJL_MAXPAIR 256
#define MJL_MAXSENSOR 4
#define MJL_MAXRSENSOR 128
#define MJL_MAXRSENSORDATA 256
#define MJL_MAXOBS 64

/* enums (MuJoCo numbering where one exists) */
enum { MJL_GEOM_PLANE = 0, MJL_GEOM_SPHERE = 2, MJL_GEOM_CAPSULE = 3, MJL_GEOM_BOX = 6 };
enum { MJL_JNT_FREE = 0, MJL_JNT_HINGE = 3 };
enum { MJL_SOLVER_CG = 1, MJL_SOLVER_NEWTON = 2 };
enum { MJL_INT_EULER = 0, MJL_INT_IMPLICITFAST = 3 };
enum { MJL_COL_PLANE_SPHERE = 0, MJL_COL_PLANE_CAPSULE = 1, MJL_COL_SPHERE_SPHERE = 2,
       MJL_COL_SPHERE_CAPSULE = 3, MJL_COL_CAPSULE_CAPSULE = 4 };
/* Sensor types and object types of the readout table (mjlModelDesc.rsensor_*, mjl_sensors). The numbering is
 * this project's own, not MuJoCo's mjtSensor / mjtObj; MJL_SENS_TOUCH stays 0. Stage of each type
 * (mj_sensorPos / mj_sensorVel / mj_sensorAcc): pos = JOINTPOS, FRAMEPOS, FRAMEQUAT, FRAME[XYZ]AXIS; vel =
 * JOINTVEL, GYRO, VELOCIMETER, FRAMELINVEL, FRAMEANGVEL; acc = TOUCH, ACCELEROMETER, ACTUATORFRC,
 * JOINTACTUATORFRC, JOINTLIMITFRC. MJL_OBJ_TOUCH: the object is an entry of the touch list (sensor_*). */
enum { MJL_SENS_TOUCH = 0, MJL_SENS_JOINTPOS = 1, MJL_SENS_JOINTVEL = 2, MJL_SENS_FRAMEPOS = 3,
       MJL_SENS_FRAMEQUAT = 4, MJL_SENS_FRAMEXAXIS = 5, MJL_SENS_FRAMEYAXIS = 6, MJL_SENS_FRAMEZAXIS = 7,
       MJL_SENS_GYRO = 8, MJL_SENS_VELOCIMETER = 9, MJL_SENS_FRAMELINVEL = 10, MJL_SENS_FRAMEANGVEL = 11,
       MJL_SENS_ACCELEROMETER = 12, MJL_SENS_ACTUATORFRC = 13, MJL_SENS_JOINTACTUATORFRC = 14,
       MJL_SENS_JOINTLIMITFRC = 15, MJL_NSENSTYPE = 16 };
enum { MJL_OBJ_XBODY = 0, MJL_OBJ_SITE = 1, MJL_OBJ_JOINT = 2, MJL_OBJ_ACTUATOR = 3, MJL_OBJ_TOUCH = 4 };
enum { MJL_SENS_STAGE_POS = 1, MJL_SENS_STAGE_VEL = 2, MJL_SENS_STAGE_ACC = 4 };
enum { MJL_ACT_MOTOR = 0, MJL_ACT_GENERAL = 1 };

typedef struct mjlModelDesc {
  int32_t nq, nv, nu, nbody, njnt, ngeom, nsite, ntendon, npair, nsensor, nsensordata;
  int32_t iterations, ls_iterations, solver, integrator, eulerdamp;
  double timestep, gravity[3], impratio, tolerance, ls_tolerance, meaninertia;

  int32_t body_parentid[MJL_MAXBODY], body_rootid[MJL_MAXBODY], body_weldid[MJL_MAXBODY];
  int32_t body_jntadr[MJL_MAXBODY], body_jntnum[MJL_MAXBODY];
  int32_t body_dofadr[MJL_MAXBODY], body_dofnum[MJL_MAXBODY];
  int32_t body_subtree_end[MJL_MAXBODY], body_level[MJL_MAXBODY];
  double body_pos[MJL_MAXBODY][3], body_quat[MJL_MAXBODY][4], body_ipos[MJL_MAXBODY][3];
  double body_inertia[MJL_MAXBODY][6]; /* body-frame tensor about ipos: xx yy zz xy xz yz */
  double body_mass[MJL_MAXBODY], body_invweight0[MJL_MAXBODY][2];

  int32_t jnt_type[MJL_MAXJNT], jnt_qposadr[MJL_MAXJNT], jnt_dofadr[MJL_MAXJNT];
  int32_t jnt_bodyid[MJL_MAXJNT], jnt_limited[MJL_MAXJNT];
  double jnt_pos[MJL_MAXJNT][3], jnt_axis[MJL_MAXJNT][3], jnt_range[MJL_MAXJNT][2];
  double jnt_stiffness[MJL_MAXJNT], jnt_margin[MJL_MAXJNT];
  double jnt_solref[MJL_MAXJNT][2], jnt_solimp[MJL_MAXJNT][5];

  int32_t dof_bodyid[MJL_MAXV], dof_jntid[MJL_MAXV], dof_parentid[MJL_MAXV];
  double dof_damping[MJL_MAXV], dof_armature[MJL_MAXV], dof_invweight0[MJL_MAXV];
  double qpos0[MJL_MAXQ], qpos_spring[MJL_MAXQ];

  int32_t geom_type[MJL_MAXGEOM], geom_bodyid[MJL_MAXGEOM];
  double geom_pos[MJL_MAXGEOM][3], geom_quat[MJL_MAXGEOM][4], geom_size[MJL_MAXGEOM][3];

  int32_t pair_geom1[MJL_MAXPAIR], pair_geom2[MJL_MAXPAIR], pair_kind[MJL_MAXPAIR];
  int32_t pair_condim[MJL_MAXPAIR];
  double pair_friction[MJL_MAXPAIR][5], pair_solref[MJL_MAXPAIR][2], pair_solimp[MJL_MAXPAIR][5];
  double pair_margin[MJL_MAXPAIR], pair_gap[MJL_MAXPAIR];

  int32_t site_type[MJL_MAXSITE], site_bodyid[MJL_MAXSITE];
  double site_pos[MJL_MAXSITE][3], site_quat[MJL_MAXSITE][4], site_size[MJL_MAXSITE][3];

  int32_t actuator_trnid[MJL_MAXU], actuator_ctrllimited[MJL_MAXU];
  double actuator_gear[MJL_MAXU], actuator_ctrlrange[MJL_MAXU][2];
  /* General (stateless, affine-bias) actuators on a hinge, MJX forward.fwd_actuation with joint transmission:
   *   force = gain * clip(ctrl) + biasprm[0] + biasprm[1] * gear * qpos[j] + biasprm[2] * gear * qvel[d],
   * clipped to forcerange when forcelimited, and qfrc_actuator[d] += gear * force. Under implicitfast the
   * integrator's matrix gets -dt * gear^2 * biasprm[2] on dof d's diagonal, whether or not the force was
   * clipped (derivative.deriv_smooth_vel). actuator_kind: MJL_ACT_MOTOR (0) reads none of the four fields
   * below (gain 1, no bias, no force limit), so an all-zero group is the torque motor; MJL_ACT_GENERAL reads
   * them all. Not differentiated: see the step VJP entries and mjl_step_jacobian. */
  int32_t actuator_kind[MJL_MAXU], actuator_forcelimited[MJL_MAXU];
  double actuator_gain[MJL_MAXU], actuator_biasprm[MJL_MAXU][3], actuator_forcerange[MJL_MAXU][2];

  int32_t tendon_num[MJL_MAXTENDON], tendon_jnt[MJL_MAXTENDON][MJL_MAXTENWRAP];
  int32_t tendon_limited[MJL_MAXTENDON];
  double tendon_coef[MJL_MAXTENDON][MJL_MAXTENWRAP], tendon_range[MJL_MAXTENDON][2];
  double tendon_margin[MJL_MAXTENDON], tendon_solref[MJL_MAXTENDON][2];
  double tendon_solimp[MJL_MAXTENDON][5], tendon_invweight0[MJL_MAXTENDON];

  /* Readout table (mjl_sensors): ALL sensors in declaration order, MuJoCo's sensor ids, so adr / dim are the
   * layout of Data.sensordata [nrsensordata]. type: MJL_SENS_*; objtype: MJL_OBJ_*; objid: a body (XBODY), site,
   * joint (a hinge) or actuator id, or, for a touch sensor, its index in the touch list below; dim: 1, 3 or 4 by
   * type. Slices [adr, adr + dim) lie inside [0, nrsensordata) and do not overlap. nrsensor = 0: no readout. */
  int32_t nrsensor, nrsensordata;
  int32_t rsensor_type[MJL_MAXRSENSOR], rsensor_objtype[MJL_MAXRSENSOR], rsensor_objid[MJL_MAXRSENSOR];
  int32_t rsensor_adr[MJL_MAXRSENSOR], rsensor_dim[MJL_MAXRSENSOR];

  /* The touch list: the touch sensors the step kernels run (nsensor <= MJL_MAXSENSOR entries, nsensordata their
   * width, MJL_FIELD_SENSORDATA their values; the env config's touch ids index it). It closes the struct. */
  int32_t sensor_type[MJL_MAXSENSOR], sensor_objid[MJL_MAXSENSOR], sensor_adr[MJL_MAXSENSOR];
} mjlModelDesc;

/* Env configuration: EnvConfig (reference src/config.py:29-66) with the flip permutation
 * tables already expanded the way create_env_functions builds them (src/envs.py:48-74). */
typedef struct mjlEnvConfig {
  float progress_weight, electricity_cost, stall_torque_cost, posture_penalty_weight;
  float tall_height_threshold, tall_bonus_weight, target_threshold, target_dist;
  float stance_time_reward_weight, random_joint_noise, random_vel_noise, initial_velocity_max;
  float terminate_height, terminate_reward;
  int32_t stop_frames, max_episode_steps, random_flip;
  int32_t pelvis_body_id, head_body_id, touch_sensor_right_id, touch_sensor_left_id;
  int32_t obs_dim;
  int32_t act_perm[MJL_MAXU];
  float act_sign[MJL_MAXU];
  int32_t obs_perm[MJL_MAXOBS];
  float obs_sign[MJL_MAXOBS];
} mjlEnvConfig;

#define MJL_AUX_DIM 9 /* [flip, tx, ty, tz, close_count, stance, stance_time, last_pot, episode_step] */

/* error codes */
enum { MJL_OK = 0, MJL_ERR_ARG = 1, MJL_ERR_UNSUPPORTED = 2, MJL_ERR_HIP = 3, MJL_ERR_NOGPU = 4 };

/* readable per-env fields (mjl_get / mjl_set) */
enum {
  MJL_FIELD_QPOS = 0,          /* [nq]   Data.qpos */
  MJL_FIELD_QVEL = 1,          /* [nv]   Data.qvel */
  MJL_FIELD_QACC_WARMSTART = 2,/* [nv]   Data.qacc_warmstart */
  MJL_FIELD_TIME = 3,          /* [1]    Data.time */
  MJL_FIELD_CTRL = 4,          /* [nu]   Data.ctrl */
  MJL_FIELD_QACC = 5,          /* [nv]   Data.qacc (constrained forward acceleration) */
  MJL_FIELD_XPOS = 6,          /* [nbody*3] Data.xpos (from the last forward pass) */
  MJL_FIELD_XQUAT = 7,         /* [nbody*4] Data.xquat */
  MJL_FIELD_QFRC_ACTUATOR = 8, /* [nv]   Data.qfrc_actuator */
  MJL_FIELD_SENSORDATA = 9,    /* [nsensordata] Data.sensordata */
  MJL_FIELD_AUX = 10,          /* [9]    env aux state (src/envs.py:15) */
  MJL_FIELD_STATS = 11,        /* [4]    ncon_active, nefc_active, solver_iter, and nan_flag (env
                                          step) or the mean active rows per Newton Hessian (others) */
  MJL_FIELD_QFRC_BIAS = 12,    /* [nv]   Data.qfrc_bias */
  MJL_FIELD_QFRC_PASSIVE = 13, /* [nv]   Data.qfrc_passive */
  MJL_FIELD_QFRC_CONSTRAINT = 14, /* [nv] Data.qfrc_constraint */
  MJL_FIELD_QACC_SMOOTH = 15,  /* [nv]   Data.qacc_smooth */
  MJL_NFIELD = 16
};

typedef struct mjlModel mjlModel;
typedef struct mjlBatch mjlBatch;

/* Message of the last failing call on this thread. */
const char* mjl_last_error(void);
/* Library version string, "mjx355 <version> (gfx950) src=<hash>": <hash> is the sha256 prefix of the
   sources the library was built from (mjx_amd/_srchash.py); loaders compare it with their tree. */
const char* mjl_version(void);

/* Replaces mjx.put_model(MjModel) (src/training_utils.py:105): validate + upload constants.
 * Host only; does not need a GPU until mjl_batch_create. */
int mjl_model_create(const mjlModelDesc* desc, mjlModel** out);
void mjl_model_destroy(mjlModel* model);
/* Max constraint rows the model can produce (contacts + limits); sizes per-env scratch. */
int mjl_model_nefc_max(const mjlModel* model);
/* Max contacts one env can produce (one per candidate pair, two per plane-capsule pair). */
int mjl_model_ncon_max(const mjlModel* model);

/* Replaces the batched mjx.make_data pytree (src/envs.py:110): owns per-env state on `device`,
 * initialised like make_data (qpos = qpos0, everything else zero). */
int mjl_batch_create(const mjlModel* model, int nenv, int device, mjlBatch** out);
void mjl_batch_destroy(mjlBatch* batch);
int mjl_batch_nenv(const mjlBatch* batch);

/* Batch options. MJL_OPT_STORE_DERIVED (default 1): step/env kernels also write the derived
 * per-env outputs (xpos, xquat, qacc, forces, sensordata, stats) readable with mjl_get; set 0 to
 * keep only the state + env outputs in the hot loop. MJL_OPT_FORCE_GLOBAL_ROWS (default 0, test
 * hook): keep constraint rows in the global-memory scratch even when they fit in LDS.
 * MJL_OPT_VJP_UNROLLED (default 0): the step VJPs differentiate the constraint solve's iterations
 * as executed (what jax.grad through MJX's fixed-count solver computes; reference train_apg.py:
 * 101-105,187-189 runs CG 4/4) instead of the implicit derivative at the converged active set; the
 * integrator's input is then qfrc_smooth + qfrc_constraint of the stopped solve. The VJP must see
 * the pre-step qacc_warmstart the forward step saw (the recompute replays that solve). Rejected for
 * models with iterations > 256 or ls_iterations > 31 (the tape's capacity); an env whose tape still
 * overflows gets NaN cotangents, or is cut and counted by the guarded VJPs.
 * MJL_OPT_VJP_TAPE (default 0): value = slots of the VJP tape (mjl_env_step_record /
 * mjl_env_step_vjp_replay), each holding one env step's forward workspace for every env
 * (~50 KB per env and slot for the humanoid; call outside stream capture; 0 frees it).
 * MJL_OPT_RESET_POOL (default 0): value = slots per env (<= 64) of the reset pool that
 * mjl_env_fill_reset_pool fills (call outside stream capture; 0 frees it).
 * MJL_OPT_PER_ENV_MODEL (default 0): 1 gives every env a model block of its own, filled with the
 * model's values (nenv x 46976 bytes, the size of one device model block: 96 MB for 2048 envs; call
 * outside stream capture; 0 frees them). See mjl_batch_set_model_params.
 * MJL_OPT_RAY_CHUNK (default 0, tuning hook of tools/ray_bench.py): value = rays per wavefront of mjl_ray /
 * mjl_ray_scan, 0..65535; 0 = the library's choice. The results do not depend on it.
 * MJL_OPT_LINEARIZE_GROUPS (default 0, test and tuning hook of tools/linearize_bench.py): value = row groups per
 * env of mjl_step_jacobian, 0..16; 0 = the library's choice from the env count. The results do not depend on it,
 * bit for bit.
 * MJL_OPT_DISTANCE_CHUNK (default 0, test and tuning hook of tools/distance_bench.py): value = geom pairs per
 * wavefront of mjl_geom_distance, 0..65535; 0 = the library's choice. The results do not depend on it, bit for
 * bit. */
enum { MJL_OPT_STORE_DERIVED = 0, MJL_OPT_FORCE_GLOBAL_ROWS = 1, MJL_OPT_VJP_UNROLLED = 2, MJL_OPT_RESET_POOL = 3,
       MJL_OPT_VJP_TAPE = 4, MJL_OPT_PER_ENV_MODEL = 5, MJL_OPT_RAY_CHUNK = 6, MJL_OPT_LINEARIZE_GROUPS = 7,
       MJL_OPT_DISTANCE_CHUNK = 8 };
int mjl_batch_set_option(mjlBatch* batch, int option, int value);

/* Per-env model parameters (domain randomisation; in MJX jax.vmap(step, in_axes=(model_axes, 0)) over a
 * model whose fields carry a batch axis, Brax's domain_randomize). The fields that can differ per env, each
 * float32 device rows [nenv, dim]:
 *   MJL_MP_BODY_MASS      body_mass                            dim nbody
 *   MJL_MP_BODY_INERTIA   body_inertia (xx yy zz xy xz yz)     dim nbody * 6
 *   MJL_MP_DOF_DAMPING    dof_damping                          dim nv
 *   MJL_MP_DOF_ARMATURE   dof_armature                         dim nv
 *   MJL_MP_ACTUATOR_GEAR  actuator_gear                        dim nu
 *   MJL_MP_PAIR_FRICTION  pair_friction[p][0], the mu of the pyramidal rows   dim npair
 *                         (the sliding coefficient of both tangent directions: MuJoCo's [0] and [1], always equal)
 * mjl_model_param_dim returns the dim (-1: null model or unknown id).
 * Semantics: env e runs the model whose descriptor has these fields replaced by env e's values (each taken
 * as (double)(float)) and nothing else recomputed, as sys.tree_replace under vmap, which does not re-run
 * mj_setConst: body_invweight0, dof_invweight0, tendon_invweight0 and meaninertia stay the model's; what is
 * computed from the replaced fields follows them (the subtree masses, the damping flag, the contact rows'
 * invweight (tran + mu^2 tran) 2 mu^2 / impratio). Env e's block is byte for byte the block mjl_model_create
 * makes of that descriptor.
 * mjl_batch_set_model_params: one launch, no allocation, no synchronisation, capturable; values[k] (k =
 * MJL_MP_*, a table of MJL_NMP device pointers read by the host at the call) NULL keeps every env's current
 * value of field k; envs with mask <= 0.5 keep their block (mask NULL = all); the values are read at
 * execution time. MJL_ERR_ARG for a null batch / values or when MJL_OPT_PER_ENV_MODEL is off.
 * mjl_batch_get_model_params copies field `param` of every env's block to dst [nenv, dim]: what the kernels
 * will use.
 * While the option is on, mjl_forward, mjl_forward_contacts, mjl_step, mjl_env_step (its in-kernel
 * auto-reset and pooled resets included), mjl_env_reset and mjl_env_fill_reset_pool run env e on its block;
 * pooled resets are computed with the blocks as they are at the fill. mjl_speedtest_step runs the model's
 * own values. Not differentiated: every step VJP, record and replay entry and mjl_step_jacobian returns
 * MJL_ERR_UNSUPPORTED while the option is on. The renderer is not concerned (no geometric field). */
#define MJL_NMP 6
enum { MJL_MP_BODY_MASS = 0, MJL_MP_BODY_INERTIA = 1, MJL_MP_DOF_DAMPING = 2, MJL_MP_DOF_ARMATURE = 3,
       MJL_MP_ACTUATOR_GEAR = 4, MJL_MP_PAIR_FRICTION = 5 };
int mjl_model_param_dim(const mjlModel* model, int param);
int mjl_batch_set_model_params(mjlBatch* batch, const float* const* values, const float* mask, void* stream);
int mjl_batch_get_model_params(mjlBatch* batch, int param, float* dst, void* stream);

/* Copy a per-env field to / from a device buffer [nenv, dim] (async on stream). `mask` (device,
 * float [nenv], may be NULL) restricts mjl_set to envs with mask > 0.5. */
int mjl_get(mjlBatch* batch, int field, float* dst, void* stream);
int mjl_set(mjlBatch* batch, int field, const float* src, const float* mask, void* stream);

/* Replaces mjx.forward (src/envs.py:112): full forward pass, no integration, on envs with
 * mask > 0.5 (mask may be NULL = all). Results readable via mjl_get. */
int mjl_forward(mjlBatch* batch, const float* mask, void* stream);

/* mjl_forward on envs with mask > 0.5 (NULL = all), then the contacts of that forward pass.
 * Replaces reading Data.contact and mj_contactForce after mjx.forward.
 * Per env, contacts c < min(ncon[env], max_con) in the kernel's emission order, which is also the
 * order of their constraint rows. Entries c >= ncon[env] are filled: geom = -1, the rest 0.
 * ncon      int32 [nenv]               true count, also when it exceeds max_con; required
 * geom      int32 [nenv, max_con, 2]   geom1, geom2
 * dim       int32 [nenv, max_con]      condim (1 or 3)
 * efc_adr   int32 [nenv, max_con]      first constraint row of the contact
 * dist      float [nenv, max_con]      signed distance
 * pos       float [nenv, max_con, 3]   world position
 * frame     float [nenv, max_con, 9]   rows: normal from geom1 to geom2, tangent 1, tangent 2
 * force     float [nenv, max_con, 3]   contact-frame force (normal, t1, t2), mj_contactForce:
 *                                      pyramidal: normal = sum of the rows' forces,
 *                                      t_i = (f[2i] - f[2i+1]) mu; condim 1: (f, 0, 0)
 * body_force float [nenv, nbody, 3]    net world-frame contact force on each body: +F on geom2's
 *                                      body, -F on geom1's (body 0 = world), F = frame^T force,
 *                                      summed over ALL ncon contacts whatever max_con is, in contact order
 * Every output but ncon may be NULL. Envs outside the mask keep their output rows untouched.
 * No allocation, no synchronisation, capturable. MJL_ERR_ARG: null batch / ncon, max_con < 1. */
int mjl_forward_contacts(mjlBatch* batch, const float* mask, int max_con, int32_t* ncon, int32_t* geom,
                         int32_t* dim, int32_t* efc_adr, float* dist, float* pos, float* frame, float* force,
                         float* body_force, void* stream);

/* Sensor readout: Data.sensordata of the batch's current state, every sensor of the model's readout table
 * (mjlModelDesc.rsensor_*) as MuJoCo defines it (mj_sensorPos / mj_sensorVel / mj_sensorAcc; MJX sensor.py for
 * the types it has). out: float [nenv, nrsensordata], sensor s of env e at out[e, adr[s] : adr[s] + dim[s]].
 * With R, p the rotation and origin of the sensor's frame (an xbody: xpos / xquat; a site), w the angular
 * velocity of the carrying body, p', p'' the classical world-frame velocity and acceleration of the point p:
 *   pos  JOINTPOS qpos[jnt_qposadr]; FRAMEPOS p; FRAMEQUAT the unit quaternion of R; FRAME[XYZ]AXIS R's columns
 *   vel  JOINTVEL qvel[jnt_dofadr]; GYRO R' w; VELOCIMETER R' p'; FRAMELINVEL p'; FRAMEANGVEL w
 *   acc  TOUCH as MJL_FIELD_SENSORDATA; ACCELEROMETER R' (p'' - gravity) with Data.qacc; ACTUATORFRC the
 *        actuator's scalar force after the force-range clamp; JOINTACTUATORFRC qfrc_actuator[dof];
 *        JOINTLIMITFRC efc_force of the joint's limit row, 0 while the limit is inactive
 * stages: a mask of MJL_SENS_STAGE_*; slots of sensors whose stage is not in it keep their content. Envs with
 * mask <= 0.5 keep their rows (mask NULL = all envs).
 * With MJL_SENS_STAGE_ACC the call first runs mjl_forward on the masked envs (applied forces and per-env model
 * parameters take part as they do there, and the derived fields are left as that forward leaves them), so
 * POS | VEL | ACC is mjx.forward(d).sensordata of the current state. Without it the call is one launch that
 * reads qpos / qvel and the model only and writes nothing but out: the call to make after mjl_env_step for
 * observations of the post-step state. ACTUATORFRC reads the env's own model block while
 * MJL_OPT_PER_ENV_MODEL is on (the gear enters the force).
 * No allocation, no synchronisation, capturable. MJL_ERR_ARG: null batch / out, stages 0 or with unknown bits.
 * A model without readout sensors returns MJL_OK and launches nothing.
 * mjl_model_nrsensordata: the row width (-1 for a null model). */
int mjl_model_nrsensordata(const mjlModel* model);
int mjl_sensors(mjlBatch* batch, const float* mask, int stages, float* out, void* stream);

/* Body-level Data readout of the batch's current state: mjx.Data's xipos, ximat, subtree_com, cinert, cvel,
 * subtree_linvel, subtree_angmom, cfrc_ext and cfrc_int. Every output is float32 on the device, [nenv, nbody, k]
 * with k = 3, 9, 3, 10, 6, 3, 3, 6, 6 in the order of the arguments; an output passed as NULL is not wanted and
 * costs nothing. All quantities are in the world frame. With b a body, k ranging over subtree(b) = [b,
 * body_subtree_end[b]), c0 = subtree_com[body_rootid[b]], R_k / x_k the body frame, w_k / dw_k its angular velocity
 * and acceleration, v_k / a_k the classical velocity and acceleration of the body's centre of mass xipos_k, T_k the
 * body-frame tensor body_inertia, I_k = R_k T_k R_k' (= ximat_k diag(principal moments) ximat_k') and g gravity:
 *   pos  xipos           xpos + xmat body_ipos
 *        ximat           xmat quat2mat(body_iquat), row-major; body_iquat: the principal axes of T_b, the moments
 *                        in descending order, a proper rotation (moments that coincide leave the axes within their
 *                        eigenspace to the library: the body axes where T_b is diagonal). Row 0: the identity
 *        subtree_com[b]  sum_k m_k xipos_k / sum_k m_k; row 0 is the whole model; a massless subtree gives xipos_b
 *        cinert[b]       MuJoCo's 10-vector: [0..5] the rotational inertia about c0 in the order (xx, yy, zz, xy,
 *                        xz, yz), I_b + m_b (|r|^2 1 - r r') with r = xipos_b - c0; [6..8] m_b r; [9] m_b
 *   vel  cvel[b]         [w_b ; velocity of the body-fixed point at c0]: MuJoCo's com-based spatial velocity
 *        subtree_linvel[b]  sum_k m_k v_k / sum_k m_k (0 for a massless subtree)
 *        subtree_angmom[b]  sum_k [ I_k w_k + m_k (xipos_k - subtree_com_b) x (v_k - subtree_linvel_b) ]: the
 *                        angular momentum about the subtree's own centre of mass
 *   acc  cfrc_ext[b]     [torque about c0 ; force] of the external loads on body b alone: its attached xfrc_applied
 *                        row (the force at xipos_b, plus its torque) and every contact force of the forward pass,
 *                        acting at the contact's pos: + frame' force on geom2's body and the opposite on geom1's
 *                        (mjl_forward_contacts' convention); a contact with the world loads the moving side only
 *        cfrc_int[b]     sum_k { [ I_k dw_k + w_k x I_k w_k + (xipos_k - c0) x m_k (a_k - g) ; m_k (a_k - g) ]
 *                        - cfrc_ext[k] }: the wrench the parent exerts on b through their joint, about c0, what
 *                        mj_rnePostConstraint accumulates (MuJoCo's force / torque sensors). A free root's is 0
 *                        up to the solver's residual (qfrc_applied, a generalized force, is not a body load)
 * Row 0 (the world) of cinert, cvel, cfrc_ext and cfrc_int is zero.
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs).
 * With neither cfrc output the call is one launch that reads qpos / qvel and the model only and writes nothing but
 * the outputs: the call to make after mjl_env_step. With one, the call first runs mjl_forward on the masked envs
 * (applied forces and per-env model parameters take part as they do there, and the derived fields are left as that
 * forward leaves them), then reads its qacc and contacts.
 * While MJL_OPT_PER_ENV_MODEL is on, body_mass, body_inertia (T_k) and body_ipos are the env's own block's;
 * body_iquat stays the model's (a per-env tensor enters I_k in full, whatever its axes).
 * No allocation, no synchronisation, capturable. MJL_ERR_ARG: null batch, or all nine outputs NULL. */
int mjl_body_data(mjlBatch* batch, const float* mask,
                  float* xipos, float* ximat, float* subtree_com, float* cinert,      /* pos */
                  float* cvel, float* subtree_linvel, float* subtree_angmom,           /* vel */
                  float* cfrc_ext, float* cfrc_int,                                    /* acc */
                  void* stream);

/* Point Jacobians of the batch's current state: mj_jac / mjx's support.jac for npoint points per env, each carried
 * by a body. Buffers (float32 / int32, device, read at execution time): body [npoint], shared by all envs; jacp,
 * jacr [nenv, npoint, 3, nv] row-major (MuJoCo's 3 x nv layout), either may be NULL, not both; xpnt
 * [nenv, npoint, 3], the world point used, or NULL.
 *   MJL_JAC_WORLD  pnt [nenv, npoint, 3]: world points, as in mj_jac(m, d, point, body).
 *   MJL_JAC_LOCAL  pnt [npoint, 3]: offsets in the body's frame, the world point is xpos_b + R_b pnt; NULL: the
 *                  body origins. A site is its body with pnt = site_pos.
 * Poses: forward kinematics of the batch's current qpos, run in the same launch, the free joint's quaternion
 * normalised as the step normalises it (the rays' rule). No mjl_forward is needed first, the stored xpos / xquat
 * are neither read nor written, so the call is correct right after mjl_env_step. Per-env model parameters and
 * applied forces do not matter (no geometric field is per-env).
 * Column d is zero unless dof d moves the body (a dof of the body or of one of its ancestors). For such a dof,
 * with x the point:
 *   hinge, world axis a through the world anchor p     jacr[:, d] = a         jacp[:, d] = a x (x - p)
 *   free joint, translation i                          jacr[:, d] = 0         jacp[:, d] = e_i
 *   free joint, rotation i (body-local rates)          jacr[:, d] = R_b e_i   jacp[:, d] = (R_b e_i) x (x - xpos_b)
 * so jacp qvel is the world velocity of the point and jacr qvel the body's angular velocity: what mjl_sensors
 * (framelinvel, frameangvel) and mjl_body_data (cvel) report. Body 0 gives zero rows. A body id outside
 * 0..nbody-1 gives NaN rows in jacp, jacr and xpnt (mjl_gather_rows' rule for a bad index).
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs). One launch, no allocation, no synchronisation,
 * capturable. MJL_ERR_ARG: a null batch or body; jacp and jacr both NULL; npoint outside 1..256; an unknown frame;
 * pnt NULL with MJL_JAC_WORLD. */
enum { MJL_JAC_WORLD = 0, MJL_JAC_LOCAL = 1 };
int mjl_jac(mjlBatch* batch, const float* mask, int npoint, const int32_t* body, int frame, const float* pnt,
            float* jacp, float* jacr, float* xpnt, void* stream);

/* The joint-space inertia of the batch's current qpos, products and solves with it: mj_fullM / support.full_m,
 * support.mul_m and smooth.solve_m. Buffers (float32, device): full_m [nenv, nv, nv], dense; vec, mul_m, solve_m
 * [nenv, nvec, nv]. Any output may be NULL, not all three; vec is required with mul_m or solve_m; nvec in 0..64,
 * 0 only with full_m alone.
 *   full_m[e]      M_e: the composite-rigid-body matrix, dof_armature on the diagonal; symmetric bit for bit
 *   mul_m[e, k]    M_e vec[e, k]
 *   solve_m[e, k]  M_e^-1 vec[e, k], by a Cholesky factor of M_e computed in the kernel
 * Poses as mjl_jac: forward kinematics of the current qpos in the same launch, nothing of the batch read but qpos
 * or written. While MJL_OPT_PER_ENV_MODEL is on, env e uses its own block's body_mass, body_inertia, body_ipos
 * and dof_armature.
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs). One launch, no allocation, no synchronisation,
 * capturable. MJL_ERR_ARG: a null batch; every output NULL; nvec outside 0..64; mul_m or solve_m with vec NULL or
 * nvec = 0. */
int mjl_mass_matrix(mjlBatch* batch, const float* mask, float* full_m, int nvec, const float* vec, float* mul_m,
                    float* solve_m, void* stream);

/* Time derivatives of mjl_jac's point Jacobians and the velocity-product term of a task acceleration
 * (xdd = J qacc + Jdot qvel): mj_jacDot for npoint points per env. npoint, body, frame (MJL_JAC_WORLD /
 * MJL_JAC_LOCAL) and pnt are exactly mjl_jac's; a MJL_JAC_WORLD point is attached to its body at this instant.
 * Buffers (float32, device): jacp_dot, jacr_dot [nenv, npoint, 3, nv] row-major; jdotv [nenv, npoint, 6] =
 * (jacp_dot qvel ; jacr_dot qvel), the point's classical acceleration and the body's angular acceleration at
 * qacc = 0. Any output may be NULL, not all three; jdotv alone is the cheap call (no nv-wide stores).
 * The outputs are the derivatives of mjl_jac's outputs along the motion qpos(t) whose rate is the batch's qvel
 * (positions integrate as the step integrates them, the free joint's angular rates body-local), the point fixed
 * in its body. With a_d, p_d the world axis and anchor of dof d as mjl_jac defines them, x the point and
 * xd = jacp qvel its velocity, column d is zero unless dof d moves the body, and for such a dof:
 *   hinge                      ad = w x a_d, pd = v(p_d): w and v(.) the angular velocity and the velocity field
 *                              of the dofs that precede d on its chain (earlier hinges of the same body, every
 *                              dof of the ancestor bodies; including d itself changes nothing)
 *   free joint, translation i  both columns are zero
 *   free joint, rotation i     ad = (R_b qvel_rot) x (R_b e_i): the axis turns with the body's whole angular
 *                              velocity; pd = qvel_lin
 *   in every moving case       jacr_dot[:, d] = ad      jacp_dot[:, d] = ad x (x - p_d) + a_d x (xd - pd)
 * jdotv is the product of these columns with qvel, summed in the kernel. With qvel = 0 every output is exactly
 * zero. Body 0 gives zero rows; a body id outside 0..nbody-1 gives NaN rows (mjl_jac's rule).
 * Poses and rates: forward kinematics of the batch's current qpos / qvel, run in the same launch; nothing of the
 * batch is read but qpos and qvel, nothing written, so the call is correct right after mjl_env_step. Per-env
 * model parameters and applied forces do not matter (no geometric field is per-env).
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs). One launch, no allocation, no synchronisation,
 * capturable. MJL_ERR_ARG: a null batch or body; all three outputs NULL; npoint outside 1..256; an unknown frame;
 * pnt NULL with MJL_JAC_WORLD. */
int mjl_jac_dot(mjlBatch* batch, const float* mask, int npoint, const int32_t* body, int frame, const float* pnt,
                float* jacp_dot, float* jacr_dot, float* jdotv, void* stream);

/* Centroidal quantities of nsub subtrees per env: the Jacobian of the subtree's centre of mass
 * (mj_jacSubtreeCom), the angular-momentum matrix about that centre (mj_angmomMat) and their bias. Buffers
 * (float32 / int32, device, read at execution time): body [nsub], nsub in 1..32, the subtree roots, shared by all
 * envs, 0 = the whole model; jac_com, angmom_mat [nenv, nsub, 3, nv] row-major; bias [nenv, nsub, 6]. Any output
 * may be NULL, not all three. With S(b) = [b, body_subtree_end[b]), m_b = sum_k m_k over S(b), c_b =
 * subtree_com[b], and jacp_k / jacr_k mjl_jac's Jacobians of body k at xipos_k:
 *   jac_com[b]     sum_k m_k jacp_k / m_b
 *   angmom_mat[b]  sum_k [ I_k jacr_k + m_k (xipos_k - c_b) x jacp_k ], I_k the world inertia as mjl_body_data
 *                  defines it: the angular momentum about the subtree's own centre of mass
 *   bias[b]        ( d/dt(jac_com) qvel ; d/dt(angmom_mat) qvel ) = ( sum_k m_k a_k / m_b ; sum_k [ I_k dw_k +
 *                  w_k x I_k w_k + m_k (xipos_k - c_b) x a_k ] ): the acceleration of the centre of mass and the
 *                  rate of the angular momentum at qacc = 0 (a_k, dw_k: the velocity-product accelerations)
 * so jac_com qvel = subtree_linvel[b] and angmom_mat qvel = subtree_angmom[b] of mjl_body_data. A massless
 * subtree gives zero rows; a body id outside 0..nbody-1 gives NaN rows.
 * Poses and rates as mjl_jac_dot: from the batch's current qpos / qvel in the same launch, nothing written. While
 * MJL_OPT_PER_ENV_MODEL is on, env e uses its own block's body_mass, body_inertia and body_ipos, as
 * mjl_mass_matrix does.
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs). One launch, no allocation, no synchronisation,
 * capturable. MJL_ERR_ARG: a null batch or body; nsub outside 1..32; every output NULL. */
int mjl_centroidal(mjlBatch* batch, const float* mask, int nsub, const int32_t* body, float* jac_com,
                   float* angmom_mat, float* bias, void* stream);

/* Inverse dynamics of the batch's current state: mj_inverse / mjx.inverse. Given qpos, qvel and an acceleration,
 * the generalized force that produces it, with limits and contacts. Buffers (float32, device, read at execution
 * time): qacc [nenv, nv], NULL = the batch's stored MJL_FIELD_QACC (as mj_inverse reads d->qacc); qfrc_inverse
 * [nenv, nv], required; qfrc_constraint [nenv, nv] or NULL.
 *   M, qfrc_bias, qfrc_passive  the position and velocity stages of mjl_forward on the current qpos / qvel
 *   J, D, aref                  the constraint rows of mjl_forward: joint and tendon limits, frictionless and
 *                               pyramidal contacts
 *   a_c                         the acceleration the formulas below use. Without MJL_INV_DISCRETE: qacc. With it,
 *                               qacc is read as the finite difference (qvel' - qvel) / timestep of a step and
 *                               a_c = qacc + timestep M^-1 (k o qacc) is the continuous-time acceleration the
 *                               integrator's linear solve maps to it: k[d] = dof_damping[d], under implicitfast
 *                               additionally - sum_u gear_u^2 biasprm_u[2] over the general actuators on dof d.
 *                               k applies under the integrator's own condition (implicitfast, or Euler with
 *                               eulerdamp, and any damping; implicitfast with some biasprm[2] != 0); when it does
 *                               not hold, a_c = qacc
 *   jar = J a_c - aref          efc_force_r = -D_r jar_r where jar_r < 0, else 0 (every row kind is one-sided):
 *                               the constraint update at a given acceleration, no solver iteration
 *   qfrc_constraint             J' efc_force
 *   qfrc_inverse                M a_c + qfrc_bias - qfrc_passive - qfrc_constraint
 * qfrc_inverse is the total of actuator and applied force the motion needs: after mjl_forward, with qacc NULL,
 * it equals qfrc_actuator + qfrc_applied + sum_b J_b' xfrc_applied[b] up to the solver's residual. ctrl and the
 * attached applied forces are not read. While MJL_OPT_PER_ENV_MODEL is on, env e uses its own model block, as
 * mjl_forward does.
 * Read: qpos, qvel, the model, qacc (or the stored one). Written: the outputs, nothing else of the batch: the
 * state, qacc_warmstart and every stored derived field (xpos, qfrc_*, sensordata, stats) stay bit for bit. The
 * constraint rows live in the launch's on-chip memory; when they overflow it, or with MJL_OPT_FORCE_GLOBAL_ROWS,
 * in the batch's per-env row scratch, which the call then overwrites. No entry reads that scratch across calls
 * (mjl_forward_contacts, mjl_sensors and mjl_body_data fill it and read it within one call, in stream order).
 * Envs with mask <= 0.5 keep their rows (mask NULL = all envs). One launch, no solver, no sensors; no allocation,
 * no synchronisation, capturable. MJL_ERR_ARG: a null batch; qfrc_inverse NULL; unknown flag bits. */
enum { MJL_INV_DISCRETE = 1 };
int mjl_inverse(mjlBatch* batch, const float* mask, const float* qacc, int flags, float* qfrc_inverse,
                float* qfrc_constraint, void* stream);

/* Ray casts against the batch's current state: mjx.ray / mj_ray (mjl_ray, caller-chosen world rays per env) and
 * ray patterns carried by a body or site frame (mjl_ray_scan: height scanner, lidar fan, rangefinder).
 * Buffers (float32 / int32, device): mjl_ray pnt, vec [nenv, nray, 3] in the world frame; mjl_ray_scan lpnt, lvec
 * [nray, 3] in the frame; dist [nenv, nray]; geomid [nenv, nray] or NULL; hitpos [nenv, nray, 3] or NULL.
 * Geometry: the geoms are posed by forward kinematics of the batch's current qpos, run in the same launch. No
 * mjl_forward is needed first, the stored xpos / xquat are neither read nor written, so the call is correct
 * right after mjl_env_step; it costs about what mjl_sensors with stages = pos costs. Per-env model parameters
 * and applied forces do not matter (no geometric field is per-env).
 * One ray: the smallest parameter t >= 0 with pnt + t vec on the surface of a geom that passes the filter, at
 * most cutoff when cutoff > 0 (else unbounded). vec need not be unit length (t is found along vec / |vec| and
 * scaled by 1 / |vec|; a zero vec misses); dist = t is in metres when it is. Per geom the renderer's closed
 * forms: a plane's crossing; a sphere's or capsule's near crossing, or the far one when the near one lies behind
 * the origin, so a ray that starts inside reports the exit point. geomid = the geom, ties going to the lower
 * id. A miss: dist = -1, geomid = -1 (mj_ray's convention).
 * Filter: geoms of body `bodyexclude` are skipped (-1: none); geoms of body 0 (the floor) are skipped unless
 * flags has MJL_RAY_STATIC.
 * mjl_ray_scan: the frame of objtype (MJL_OBJ_XBODY or MJL_OBJ_SITE) / objid, rotation R and origin p as the
 * pos-stage sensors define them; lpnt / lvec [nray, 3] are shared by all envs.
 *   MJL_SCAN_POSE  ray r is pnt = p + R lpnt[r], vec = R lvec[r]. A rangefinder is one ray with lpnt = 0,
 *                  lvec = +z on a site, bodyexclude = the site's body.
 *   MJL_SCAN_YAW   R is replaced by the rotation about world z by psi = atan2(R[1][0], R[0][0]) (psi = 0 when
 *                  R[0][0]^2 + R[1][0]^2 < 1e-12): a grid that turns with the heading but stays level.
 * hitpos = pnt + dist * vec in the world, pnt on a miss.
 * Envs with mask <= 0.5 keep their output rows (mask NULL = all envs). All pointers are device pointers read at
 * execution time. One launch, no allocation, no synchronisation, capturable.
 * MJL_ERR_ARG: a null batch, dist, pnt, vec, lpnt or lvec; nray outside 1..65535; unknown flag bits or align;
 * objtype other than the two above or objid out of range; bodyexclude outside -1..nbody-1.
 * MJL_ERR_UNSUPPORTED: a model with a geom that is no plane, sphere or capsule (the renderer's rule). */
enum { MJL_RAY_STATIC = 1 };
enum { MJL_SCAN_POSE = 0, MJL_SCAN_YAW = 1 };
int mjl_ray(mjlBatch* batch, const float* mask, int nray, const float* pnt, const float* vec, int flags,
            int bodyexclude, float cutoff, float* dist, int32_t* geomid, void* stream);
int mjl_ray_scan(mjlBatch* batch, const float* mask, int objtype, int objid, int align, int nray, const float* lpnt,
                 const float* lvec, int flags, int bodyexclude, float cutoff, float* dist, int32_t* geomid,
                 float* hitpos, void* stream);

/* Signed distances between geoms of the batch's current state: mj_geomDistance (the distance / normal / fromto
 * sensors' computation) for npair geom pairs per env, with the gradient. Buffers (float32 / int32, device, read at
 * execution time): geom1, geom2 [npair], shared by all envs; dist [nenv, npair], required; fromto [nenv, npair, 6],
 * normal [nenv, npair, 3], jac [nenv, npair, nv], each may be NULL (a NULL output costs no stores).
 * Geometry: the geoms are posed by forward kinematics of the batch's current qpos, run in the same launch
 * (mjl_jac's tree pass). No mjl_forward is needed first, the stored xpos / xquat are neither read nor written, so
 * the call is correct right after mjl_env_step. While MJL_OPT_PER_ENV_MODEL is on nothing changes: no geometric
 * field is among the six per-env fields; applied forces do not matter either.
 *   dist    the signed distance between the two surfaces, negative when the geoms overlap
 *   fromto  [0:3] `from`, on geom1's surface; [3:6] `to`, on geom2's, whatever the order of the two types
 *   normal  the unit vector from geom1 towards geom2: to = from + dist * normal, also when dist < 0
 *   jac     normal' (jacp(to, body of geom2) - jacp(from, body of geom1)), jacp as mjl_jac defines it: jac qvel is
 *           the rate of dist
 * Closed forms per pair of types (float32):
 *   plane - sphere / capsule  the plane is its half-space. The capsule's axis end nearer to the plane decides (a
 *                             sphere's centre; equal ends: the +z end): dist = (end - plane point) . plane normal - r,
 *                             the geom's witness is end - r plane normal, the plane's is that point's foot on the
 *                             plane, normal = +- the plane's normal (+ when the plane is geom1)
 *   sphere / capsule pairs    pa, pb the closest points of the two axis segments (a sphere's is its centre): dist =
 *                             |pb - pa| - (r1 + r2), normal = (pb - pa) / |pb - pa|, from = pa + r1 normal, to = pb -
 *                             r2 normal. Parallel axes have a segment of closest points; one pair of them is returned
 *   coincident axis points    (|pb - pa|^2 <= 1e-30: no direction is defined) dist = -(r1 + r2) exactly, normal =
 *                             world +z (0, 0, 1), from / to as above
 * distmax: when the distance exceeds it, dist = distmax and fromto, normal and jac of the pair are zeros, as MuJoCo
 * returns; +inf switches the cap off.
 * A pair whose ids are out of 0..ngeom-1, equal, or both planes gets dist = NaN and zeros in fromto, normal and
 * jac; the ids are checked in the kernel before anything is read through them (they are device memory, the host
 * cannot check them).
 * Envs with mask <= 0.5 keep their output rows (mask NULL = all envs). One launch, no allocation, no
 * synchronisation, capturable.
 * MJL_ERR_ARG: a null batch, dist, geom1 or geom2; npair outside 1..65535; distmax not greater than 0, or NaN.
 * MJL_ERR_UNSUPPORTED: a model with a geom that is no plane, sphere or capsule (the rays' rule). */
int mjl_geom_distance(mjlBatch* batch, const float* mask, int npair, const int32_t* geom1, const int32_t* geom2,
                      float distmax, float* dist, float* fromto, float* normal, float* jac, void* stream);

/* Replaces mjx.step (src/envs.py:345): ctrl (device [nenv, nu], may be NULL = keep current)
 * -> forward + integrate, state updated in place. */
int mjl_step(mjlBatch* batch, const float* ctrl, void* stream);

/* Physics substeps: the state and the stored derived fields that nstep consecutive mjl_step(batch, ctrl) leave,
 * in one call. The same ctrl holds for every substep (NULL = the stored one), and so do attached applied forces;
 * per-env model blocks are honoured; an env whose rows overflow in one substep takes the global path for that
 * substep only. The call issues nstep single-step launches on the stream (a fused launch that kept the state on
 * chip measured slower and was dropped: DESIGN.md section 3, "Substeps"); nstep == 1 is mjl_step.
 * No allocation, no synchronisation, capturable. Not differentiated: the VJP, record and replay entries stay
 * single-step. MJL_ERR_ARG: null batch, nstep outside 1..MJL_MAXSUBSTEP (the state is left untouched). */
#define MJL_MAXSUBSTEP 64
int mjl_step_n(mjlBatch* batch, const float* ctrl, int nstep, void* stream);

/* Speed-test step (mjx_humanoid_speed_test.py:48-57): for each env e, a fresh make_data state
 * with qvel[0] = vel[e], one step, out[e] = new qpos[0]. Stateless: does not touch the batch
 * state (the batch only provides scratch and the model). */
int mjl_speedtest_step(mjlBatch* batch, const float* vel, float* out, void* stream);

/* Replaces create_env_functions' EnvConfig capture (src/envs.py:26-87). */
int mjl_env_config(mjlBatch* batch, const mjlEnvConfig* cfg);

/* Replaces v_step (src/envs.py:333-495) fused with the PPO auto-reset merge
 * (train_ppo.py:147-161): act [nenv, nu] -> obs [nenv, obs_dim], rew/term/trunc [nenv].
 * If auto_reset != 0, envs with max(term, trunc) > 0.5 are re-initialised in the same launch
 * (single_reset semantics, src/envs.py:115-202, RNG stream (seed, counter, env)) and obs holds
 * the post-reset observation, exactly as merge_if_done does; rew/term/trunc stay the step's. */
int mjl_env_step(mjlBatch* batch, const float* act, float* obs, float* rew, float* term,
                 float* trunc, int auto_reset, uint64_t seed, uint64_t counter, void* stream);

/* A control step of nstep physics steps (Brax's n_frames, Gym's frame_skip): single_step of src/envs.py with
 * mjx.step applied nstep times. The result is that of ctrl = clip(flip ? act[act_perm] * act_sign : act, -1, 1)
 * (flip from the pre-step aux[0]), nstep - 1 mjl_step(ctrl), then one mjl_env_step(act, ...): reward,
 * observation, termination, the NaN flag and the stance logic are evaluated once, after the last substep, from
 * that substep's forward pass. aux[8] (the episode step) advances by 1, time by nstep * timestep; the reward's
 * dt stays opt.timestep. Auto-reset, reset pool, key-drawn resets and the counter base as in mjl_env_step, one
 * (seed, counter) draw per call. Applied forces, per-env models and the global-rows path as in mjl_step_n.
 * nstep == 1 is mjl_env_step. No allocation, no synchronisation, capturable. Not differentiated.
 * MJL_ERR_ARG: null batch or outputs, nstep outside 1..MJL_MAXSUBSTEP, mjl_env_config not called. */
int mjl_env_step_n(mjlBatch* batch, const float* act, int nstep, float* obs, float* rew, float* term,
                   float* trunc, int auto_reset, uint64_t seed, uint64_t counter, void* stream);

/* Reset pool: the v_reset half of train_ppo.py:147-161's merge_if_done, moved off the step's
 * critical path. A reset does not depend on the state it replaces, so resets can be computed in bulk
 * (full-occupancy launches) instead of one wave at a time at the end of a finishing env's step:
 * this fills slots 0..n-1 of every env (n = min(*dev_n, slots), device int read at execution
 * time), slot j drawn from (seed, (counter + j * 2^48) ^ 2^63, env) with the same single_reset semantics
 * (src/envs.py:115-202). Each later mjl_env_step(auto_reset=1) merges a finished env's next unused
 * slot; an env whose slots are used up resets in place from (seed, step counter, env) as before.
 * Requires MJL_OPT_RESET_POOL; not for key-drawn resets (mjl_env_set_reset_keys). */
int mjl_env_fill_reset_pool(mjlBatch* batch, const int* dev_n, uint64_t seed, uint64_t counter, void* stream);

/* RNG counter base for hipGraph capture of env steps / resets: if dev_counter_base (a device
 * uint64, may be NULL to detach) is set, the kernels draw with counter = the call's `counter` +
 * *dev_counter_base read at execution time, so a captured sequence of calls with counters 1..T
 * replays with fresh draws after the caller advances the base (src/envs.py:117 splits a fresh key
 * per reset; train_ppo.py:150 draws per rollout step). Eager callers leave it unset. */
int mjl_batch_set_counter_base(mjlBatch* batch, const uint64_t* dev_counter_base);

/* Exponent-carried cotangents for the guarded env-step VJPs (mjl_env_step_vjp_guarded, _vjp_full,
 * _vjp_replay, _vjp_replay_apg). exp: device int32 [nenv], in/out, true cotangent = stored * 2^exp;
 * NULL detaches (default). threshold_log2: see DESIGN.
 * Per env, with e = exp[env] >= 0 on entry: g_qpos / g_qvel / g_qacc_ws / g_aux are read as stored at
 * 2^-e, g_rew arrives unscaled and is multiplied by 2^-e in the kernel. With m the largest magnitude among
 * the env's outputs: e = 0 and m < 2^threshold_log2 leaves outputs and exponent as they are (bit-identical
 * to the detached call); otherwise the outputs are multiplied by 2^-k, k = max(floor(log2 m), -e), and
 * exp[env] = e + k. Input cotangents whose largest magnitude is at or past 2^threshold_log2 (handed in at
 * exponent 0) are multiplied by 2^-floor(log2 of it) before the reverse passes, and that power joins e. An env the guard cuts (non-finite outputs, overflowed solve tape) and an env whose input
 * cotangents are all zero get exp[env] = 0. The first attach on a batch allocates 256 B per env (call it outside
 * stream capture); every later one is a host-side pointer set, and a captured launch reads the attached address. threshold_log2 in [0, 96], else MJL_ERR_ARG. */
int mjl_vjp_scale_attach(mjlBatch* batch, int32_t* exp, int threshold_log2);

/* jax.random key modes: element i of a draw / split is threefry2x32(key, (0, i)) (jax >= 0.5
 * default, jax_threefry_partitionable; the reference pins jax==0.7.2, requirements.txt:17), or
 * the pre-0.5 layout (threefry over iota halves). */
enum { MJL_RNG_JAX_PARTITIONABLE = 1, MJL_RNG_JAX_ORIGINAL = 2 };

/* Replaces v_reset(keys) / merge_if_done's v_reset(random.split(key_reset, num_envs)) key input
 * (src/envs.py:116-147, train_ppo.py:150-152): if dev_keys (device uint32 [nenv, 2], read at
 * execution time; NULL detaches) is set, env resets — mjl_env_reset and the auto-reset of
 * mjl_env_step — draw from env e's jax.random key exactly as single_reset does (split(key, 4);
 * uniform(k1, (nq-7,)), uniform(k2, (nv,)), bernoulli(k3, .5), uniform(k4, (), 0, v_max)) instead of
 * (seed, counter): identical reset states to MJX for identical keys. */
int mjl_env_set_reset_keys(mjlBatch* batch, const uint32_t* dev_keys, int mode);

/* Applied forces (mjx.Data.qfrc_applied / xfrc_applied): caller-owned device buffers the batch reads at
 * execution time (no copy, no allocation, capturable; update them in place). Both NULL detaches (default).
 *   qfrc_applied  float [nenv, nv]        generalized force per dof, or NULL
 *   xfrc_applied  float [nenv, nbody, 6]  per body (fx, fy, fz, tx, ty, tz) in the world frame, the force
 *                                         acting at the body's inertial position xipos; row 0 (the world)
 *                                         is ignored; or NULL
 * While attached, mjl_forward, mjl_forward_contacts, mjl_step and mjl_env_step compute
 *   qfrc_smooth = qfrc_passive - qfrc_bias + qfrc_actuator + qfrc_applied + sum_b J_b(xipos_b)' [f_b; t_b]
 * (mj_xfrcAccumulate / support.xfrc_accumulate); the qfrc_bias / qfrc_passive / qfrc_actuator readouts keep
 * their meaning. The buffers are inputs like ctrl: no kernel writes them (mjl_env_push aside) and a reset
 * does not clear them. mjl_speedtest_step, mjl_env_reset, the auto-reset inside mjl_env_step and
 * mjl_env_fill_reset_pool start from a fresh make_data and run with zero applied force.
 * Not differentiated: every step VJP, record and replay entry (mjl_step_vjp*, mjl_env_step_vjp*,
 * mjl_env_step_record*, mjl_env_step_vjp_replay*) and mjl_step_jacobian return MJL_ERR_UNSUPPORTED while anything
 * is attached.
 * A host-side pointer set; MJL_ERR_ARG for a null batch. */
int mjl_batch_attach_applied(mjlBatch* batch, const float* qfrc_applied, const float* xfrc_applied);

/* Random pushes: one launch per env step, before mjl_env_step (capturable). Writes row `body` of every
 * env of the attached xfrc_applied (required, else MJL_ERR_ARG) and nothing else of it.
 * timer int32 [nenv, 2], in/out: (steps_left of the running push, steps_to_next push). done [nenv] or NULL:
 * the previous step's max(term, trunc). Uniforms u0, u1, u2 of env e: noise[e] (float [nenv, 3]) when given,
 * else uniform01(seed, c ^ 2^62, e, i), i = 0..2, c = counter + the batch's counter base
 * (mjl_batch_set_counter_base): a stream apart from the reset and pool draws. Per env, in this order:
 *   done[e] > 0.5:    row = 0, steps_left = 0, steps_to_next = draw
 *   steps_left > 0:   steps_left -= 1, row = 0 when it reaches 0
 *   otherwise:        steps_to_next -= 1; at <= 0: row = (F cos th, F sin th, 0, 0, 0, 0), th = 2 pi u1,
 *                     F = force_lo + u2 (force_hi - force_lo), steps_left = duration, steps_to_next = draw
 * draw = interval_lo + min(floor(u0 (interval_hi - interval_lo + 1)), interval_hi - interval_lo).
 * MJL_ERR_ARG: body outside 1..nbody-1, interval_lo < 1, interval_hi < interval_lo, duration < 1, null timer. */
int mjl_env_push(mjlBatch* batch, int body, int32_t* timer, int interval_lo, int interval_hi, int duration,
                 float force_lo, float force_hi, const float* done, uint64_t seed, uint64_t counter,
                 const float* noise, void* stream);

/* jax.random.split(key, num) for n keys at once: keys uint32 [n, 2] -> out [n, num, 2] (device). */
int mjl_prng_split(const uint32_t* keys, int n, int num, int mode, uint32_t* out, void* stream);

/* Replaces v_reset (src/envs.py:115-202,494) restricted to envs with mask > 0.5 (mask may be
 * NULL = all). obs [nenv, obs_dim] is written for reset envs only. `noise` (device, may be NULL)
 * overrides the on-device RNG with explicit draws [nenv, nq-7 + nv + 2] in [0,1):
 * joint-noise uniforms, velocity-noise uniforms, flip uniform, initial-speed uniform. */
int mjl_env_reset(mjlBatch* batch, const float* mask, uint64_t seed, uint64_t counter,
                  const float* noise, float* obs, void* stream);

/* Reverse-mode derivative of one mjl_step (APG backward; reference train_apg.py:161-209 takes
 * jax.value_and_grad through mjx.step, src/envs.py:345). The pre-step state is the batch state
 * (qpos, qvel, qacc_warmstart, ctrl), which is not modified. Given the cotangents of the step
 * outputs g_qpos [nenv,nq], g_qvel [nenv,nv], writes the cotangents of the inputs out_qpos
 * [nenv,nq], out_qvel [nenv,nv], out_ctrl [nenv,nu]. The constraint solve is differentiated at
 * its converged active set; qacc_warmstart gets no cotangent (DESIGN.md "APG"). */
int mjl_step_vjp(mjlBatch* batch, const float* g_qpos, const float* g_qvel, float* out_qpos,
                 float* out_qvel, float* out_ctrl, void* stream);

/* VJP of one env step (src/envs.py:333-492 single_step, without the reset merge) at the batch
 * state and aux with action act [nenv,nu]: cotangents of (qpos', qvel', reward, aux') ->
 * (qpos, qvel, action, aux). g_rew [nenv], g_aux / out_aux [nenv, MJL_AUX_DIM]. */
int mjl_env_step_vjp(mjlBatch* batch, const float* act, const float* g_qpos, const float* g_qvel,
                     const float* g_rew, const float* g_aux, float* out_qpos, float* out_qvel,
                     float* out_act, float* out_aux, void* stream);

/* Guarded env-step VJP for the APG reverse sweep: as mjl_env_step_vjp, but an env whose input
 * cotangents come out non-finite (a state blowing up inside the horizon) gets all-zero outputs and
 * increments *nonfinite_count (device float, may be NULL = unguarded). */
int mjl_env_step_vjp_guarded(mjlBatch* batch, const float* act, const float* g_qpos, const float* g_qvel,
                             const float* g_rew, const float* g_aux, float* out_qpos, float* out_qvel,
                             float* out_act, float* out_aux, float* nonfinite_count, void* stream);

/* Full-state VJPs: as mjl_step_vjp / mjl_env_step_vjp_guarded, plus the carried warm start.
 * g_qacc_ws [nenv,nv] is the cotangent of the output qacc_warmstart (= the step's qacc, MJX
 * solver.solve); out_qacc_ws [nenv,nv] receives the cotangent of the input qacc_warmstart, nonzero
 * only in MJL_OPT_VJP_UNROLLED mode when the truncated solve started from it (jax.grad through the
 * Data carry sees this path; a converged solve does not depend on its seed). Either may be NULL. */
int mjl_step_vjp_full(mjlBatch* batch, const float* g_qpos, const float* g_qvel, const float* g_qacc_ws,
                      float* out_qpos, float* out_qvel, float* out_qacc_ws, float* out_ctrl, void* stream);
int mjl_env_step_vjp_full(mjlBatch* batch, const float* act, const float* g_qpos, const float* g_qvel,
                          const float* g_qacc_ws, const float* g_rew, const float* g_aux, float* out_qpos,
                          float* out_qvel, float* out_qacc_ws, float* out_act, float* out_aux,
                          float* nonfinite_count, void* stream);

/* Linearization of one mjl_step at the batch's current qpos, qvel, qacc_warmstart: the transition matrices
 * A = dx'/dx and B = dx'/du (mjd_transitionFD; jax.jacobian(mjx.step)). ctrl [nenv, nu] (device, read at execution
 * time), NULL = the stored ctrl, as mjl_step. Nothing of the batch is written. A or B may be NULL (not both): a NULL
 * output is not stored, and with A NULL the reverse passes behind ctrl's cotangent are not run.
 * flags selects the layout:
 *   MJL_JAC_TANGENT  A [nenv, 2nv, 2nv], B [nenv, 2nv, nu], state x = (dq, qvel) in the tangent space, as
 *                    mjd_transitionFD. An input dq acts as mj_integratePos(qpos, dq, 1): hinge coordinates and a free
 *                    joint's position add, its quaternion becomes q (x) exp(d), d a rotation vector in the body
 *                    frame (linearised: dquat = 1/2 q (x) (0, d)). An output difference is mj_differentiatePos: for
 *                    the free quaternion the rotation vector of conj(q'0) (x) q' (linearised: d' = 2 vec(conj(q'0)
 *                    (x) dquat'), q'0 the post-step, normalised quaternion). Both maps are applied in the kernel.
 *   0                A [nenv, nq+nv, nq+nv], B [nenv, nq+nv, nu] in raw coordinates: row i is the derivative of
 *                    entry i of (qpos', qvel'), columns (qpos, qvel) and ctrl, as jax.jacobian(mjx.step) lays it out.
 * The constraint solve is differentiated at its converged active set (the implicit derivative of mjl_step_vjp with
 * MJL_OPT_VJP_UNROLLED off): row i of [A | B] is what mjl_step_vjp returns for the i-th basis cotangent. This
 * entry always uses the implicit form, whatever MJL_OPT_VJP_UNROLLED is set to. qacc_warmstart seeds the solver
 * and has no column.
 * One launch of one wavefront per (env, row group): the step's forward runs once per wavefront, the reverse passes
 * once per row, from cotangents formed on chip. The number of row groups per env follows from the env count
 * (MJL_OPT_LINEARIZE_GROUPS overrides it); the result does not depend on it. Envs with mask <= 0.5 keep their rows
 * of A and B (mask NULL = all envs).
 * The per-wavefront scratch (the step VJP's, times the row groups) is allocated by the first call and regrown when a
 * later call needs more (more row groups): so the first call at a given setting happens outside stream capture, and
 * a regrow invalidates graphs captured before it. After that: no allocation, no synchronisation, capturable.
 * MJL_ERR_ARG: a null batch; A and B both NULL; unknown flag bits (checked in this order, before anything else).
 * MJL_ERR_UNSUPPORTED, with the step VJPs' messages: applied forces attached, MJL_OPT_PER_ENV_MODEL on, or a model
 * with a non-motor actuator. */
enum { MJL_JAC_TANGENT = 1 };
int mjl_step_jacobian(mjlBatch* batch, const float* mask, const float* ctrl, int flags, float* A, float* B,
                      void* stream);

/* Batched inverse kinematics: a damped least-squares (Gauss-Newton) solve per env for a qpos that brings ntask body
 * or site frames to target positions and / or orientations. The whole solve, every iteration of it, is one launch
 * of one wavefront per env. Buffers (float32 / int32, device, read at execution time, row-major):
 *   body        [ntask], ntask in 1..32, shared by all envs: the carrying body of each task. A site is its body with
 *               offset = site_pos, as mjl_jac with MJL_JAC_LOCAL; an orientation target is the body frame's.
 *   offset      [ntask, 3] or NULL (the body origins): the task point in the body's frame
 *   target_pos  [nenv, ntask, 3] or NULL; target_quat [nenv, ntask, 4] or NULL (normalised on read, a zero
 *               quaternion reads as the identity): world-frame targets, not both NULL
 *   weight      [ntask, 2] or NULL: (w_pos, w_rot) per task, each >= 0; NULL = 1 where the matching target array is
 *               given. A weight that is not > 0, or a NULL target array, drops those three rows.
 *   qpos_start  [nenv, nq] or NULL (the batch's current qpos): the start of the solve
 *   qpos_ref    [nenv, nq] or NULL (the model's qpos0): the posture that `posture` pulls toward
 *   dofmask     bit d set: dof d may move; -1 (all bits) = every dof
 *   qpos_out    [nenv, nq], required: the solution; err [nenv, ntask, 6] or NULL: the unweighted residual (e_p ; e_r)
 *               at the returned qpos_out, zeros in rows without a target array; niter [nenv] or NULL: the iterations
 *               taken.
 * One iteration, all in float32 (fmaf where "fma" is written) in this order:
 *   1. Kinematics of the iterate q, as mjl_jac's: the free quaternion normalised for the pass (q itself keeps its
 *      entries), every hinge about its world axis.
 *   2. Residuals, per task t with body b: x = xpos_b + R_b offset_t, e_p = target_pos - x; q_e = target_quat (x)
 *      conj(xquat_b), negated when its scalar part is negative, e_r = its world-frame rotation vector
 *      v * (2 atan2(|v|, w) / |v|), v the vector part (zero when |v| < 1e-15): mju_quat2Vel at dt = 1.
 *      res = max_t max(w_pos |e_p|, w_rot |e_r|) over the rows that are not dropped.
 *   3. Stop: iteration k (0-based) ends the solve before its update when k = iterations, or when tol > 0 and res <
 *      tol; niter = k. The test is the same for the whole wavefront.
 *   4. Normal equations H dq = g. With Jp, Jr exactly mjl_jac's jacp, jacr of the point, the weighted rows are
 *      c_r = w J[r, :] and the weighted residuals w e[r], r = 0..5 (three position rows, then three rotation rows).
 *      H starts as (damping + posture) I and g as posture * delta. Then task by task in index order and row by row,
 *      H[i][j] = fma(c_r[i], c_r[j], H[i][j]) and g[i] = fma(c_r[i], w e[r], g[i]): both triangles of H take the
 *      same chain over the same operands, so H is symmetric bit for bit. delta = mj_differentiatePos(qpos_ref, q),
 *      the tangent from q toward the reference under the maps MJL_JAC_TANGENT documents: hinge coordinates and the
 *      free position subtract (ref - q), the free quaternion gives the body-frame rotation vector of conj(q) (x)
 *      ref (both normalised, sign as in step 2); with posture = 0 delta is not evaluated. A dof outside dofmask, or
 *      at or past nv, has the identity's row and column and g = 0.
 *   5. Step: dq = H^-1 g by mjl_mass_matrix's Cholesky factor and substitutions on the 32 x 32 matrix. When
 *      max_step > 0 and s = max_d |dq_d| > max_step, dq is multiplied by max_step / s.
 *   6. Update q <- mj_integratePos(q, dq, 1) over the dofs of dofmask: hinge coordinates and the free position add;
 *      the free quaternion becomes q (x) exp(dq_rot) in the body frame, renormalised, as the step integrates it
 *      (its entries left alone when dq_rot is zero, as it is when none of its three dofs is in dofmask or moves a
 *      task). With MJL_IK_LIMITS a limited hinge is then clamped to jnt_range.
 * iterations = 0 copies the start to qpos_out bit for bit and evaluates err. tol = 0 always runs `iterations`
 * iterations. Dofs outside dofmask keep their qpos entries bit for bit.
 * Nothing of the batch is written. Per-env model parameters and applied forces do not matter (no geometric field is
 * per-env). A body id outside 0..nbody-1 in any task gives NaN rows in qpos_out and err for every env and niter = 0
 * (mjl_jac's rule). Envs with mask <= 0.5 keep their rows of every output (mask NULL = all envs). No allocation, no
 * synchronisation, capturable.
 * MJL_ERR_ARG: a null batch, body or qpos_out; ntask outside 1..32; both target arrays NULL; iterations outside
 * 0..1024; damping <= 0, posture < 0, max_step < 0 or tol < 0 (or not finite); unknown flag bits. */
enum { MJL_IK_LIMITS = 1 };
int mjl_ik(mjlBatch* batch, const float* mask, int ntask, const int32_t* body, const float* offset,
           const float* target_pos, const float* target_quat, const float* weight, const float* qpos_start,
           const float* qpos_ref, int32_t dofmask, int iterations, float damping, float posture, float max_step,
           float tol, int flags, float* qpos_out, float* err, int32_t* niter, void* stream);

/* Whole-body inverse kinematics: mjl_ik's solve with a centre-of-mass task and one-sided geom-clearance tasks in the
 * same normal equations, still one launch of one wavefront per env. The arguments up to niter are mjl_ik's, in its
 * order and with its meaning, except that ntask may be 0 (body, offset, the targets and weight may then be NULL)
 * provided a CoM task or a pair exists. With com_body = -1 and npair = 0 qpos_out, err and niter are mjl_ik's bit
 * for bit. The added arguments:
 *   com_body      -1: no CoM task; 0: the centre of mass of the whole model; b > 0: of the subtree rooted at body b
 *   com_target    device [nenv, 3], world frame, read at execution time; required with com_body >= 0
 *   com_weight    HOST [3] or NULL (ones): one weight >= 0 per world axis; a weight that is not > 0 drops that row, so
 *                 (1, 1, 0) is "the CoM above a point on the ground"
 *   npair         0..32 clearance pairs; geom1, geom2 HOST int32 [npair]; clear_min HOST [npair], metres, >= 0;
 *                 clear_weight HOST [npair] or NULL (ones), >= 0. A plane - sphere / capsule pair is allowed (a foot
 *                 above the floor).
 *   com_err       device [nenv, 3] or NULL: e_c at the returned qpos_out, zeros in dropped rows and without a CoM task
 *   clearance     device [nenv, npair] or NULL: the signed dist of every pair at the returned qpos_out, active or not
 * The five HOST arrays are read by the host during the call and copied into the kernel's arguments (so the host can
 * refuse them, and a captured launch carries their values); every other pointer is a device pointer as in mjl_ik.
 * The iteration is mjl_ik's with these additions, all in float32:
 *   2. Residuals. CoM: with m_k, xipos_k the mass and inertial-frame origin of body k (the env's own masses while
 *      MJL_OPT_PER_ENV_MODEL is on, as mjl_centroidal), M = sum m_k and c = (sum m_k xipos_k) / M over the bodies of
 *      the subtree in id order (mjl_centroidal's sums), e_c = com_target - c. Pairs: dist_p, from, to, normal exactly
 *      as mjl_geom_distance defines them at distmax = +inf (its closed forms and degenerate-case rules), from the
 *      iterate's frames. Pair p is active iff dist_p < clear_min[p] (strict); its residual is clear_min[p] - dist_p
 *      when active, else 0. res also takes com_weight[a] |e_c[a]|, a = x, y, z, then clear_weight[p] max(0,
 *      clear_min[p] - dist_p), p in index order, after the frame tasks' terms.
 *   4. Normal equations. After the last frame task, with the same chain H[i][j] = fma(c[i], c[j], H[i][j]),
 *      g[i] = fma(c[i], w e, g[i]): the CoM rows a = x, y, z that are not dropped, c = com_weight[a] * row a of
 *      mjl_centroidal's jac_com of the subtree, w e = com_weight[a] e_c[a]; then the active pairs with clear_weight
 *      > 0 in index order, c = clear_weight[p] * (+ mjl_geom_distance's jac row of the pair), w e = clear_weight[p]
 *      (clear_min[p] - dist_p): the step increases the distance. An inactive pair adds nothing to H or g. Columns of
 *      dofs outside dofmask are zero, as for the frame rows. H stays symmetric bit for bit.
 * Steps 1, 3, 5 and 6 are unchanged; the stop test is the same for the whole wavefront. The rows are one-sided, not
 * a QP: a pair that is inactive at the iterate does not bound the step taken from it.
 * A body id outside 0..nbody-1 in a frame task gives NaN rows in qpos_out, err, com_err and clearance and niter = 0.
 * mask, "nothing of the batch is written", no allocation, no synchronisation and capturability as mjl_ik.
 * MJL_ERR_ARG, before anything touches the device: mjl_ik's refusals (ntask outside 0..32; body or both targets NULL
 * only with ntask > 0); no task of any kind; com_body outside -1..nbody-1; com_target NULL with com_body >= 0; npair
 * outside 0..32; geom1, geom2 or clear_min NULL with npair > 0; a geom id outside 0..ngeom-1, a geom paired with
 * itself, a plane - plane pair (mjl_geom_distance's rules, checked on the host here); a negative or non-finite
 * com_weight, clear_weight or clear_min.
 * MJL_ERR_UNSUPPORTED: npair > 0 on a model with a geom that is no plane, sphere or capsule. */
int mjl_ik_wb(mjlBatch* batch, const float* mask, int ntask, const int32_t* body, const float* offset,
              const float* target_pos, const float* target_quat, const float* weight, const float* qpos_start,
              const float* qpos_ref, int32_t dofmask, int iterations, float damping, float posture, float max_step,
              float tol, int flags, float* qpos_out, float* err, int32_t* niter, int com_body,
              const float* com_target, const float* com_weight, int npair, const int32_t* geom1,
              const int32_t* geom2, const float* clear_min, const float* clear_weight, float* com_err,
              float* clearance, void* stream);

/* The persistent per-env state (what a step reads and writes: Data.qpos, qvel, qacc_warmstart,
 * time, plus the env aux) as packed rows [nenv, mjl_state_size] = [qpos | qvel | qacc_warmstart |
 * aux | time]: the APG remat tape entry (train_apg.py:187-189 checkpoints each step's carry).
 * mjl_set_state takes qacc_warmstart from ws_src (same row layout, may be NULL = from src). */
int mjl_state_size(const mjlBatch* batch);
int mjl_get_state(mjlBatch* batch, float* dst, void* stream);
int mjl_set_state(mjlBatch* batch, const float* src, const float* ws_src, void* stream);

/* Replaces compute_gae (train_ppo.py:171-202, a reverse lax.scan over the rollout): rew, term,
 * trunc [T, B], val [T+1, B] (val[T] = value of the obs after the last step) -> adv, ret [T, B],
 * delta = r + gamma V' (1 - term) - V, A = delta + gamma lam (1 - max(term, trunc)) A', ret = A + V.
 * Device pointers, float32, row-major; bit-identical to the elementwise formula (no contraction). */
int mjl_gae(const float* rew, const float* val, const float* term, const float* trunc, int T, int B,
            double gamma, double lam, float* adv, float* ret, void* stream);

/* The rollout step's elementwise work around the policy GEMMs (train_ppo.py:128-169), two launches
 * instead of the ~20 framework ops it takes as jnp / torch expressions:
 * mjl_obs_normalize replaces normalize_obs + clip (src/training_utils.py:52-56, train_ppo.py:134-135):
 *   y[n, dim] = clip((x - mean) / sqrt(var + 1e-8), -clip, clip).
 * mjl_policy_head replaces GaussianPolicy's tanh head + sampling + gaussian_logprob
 * (src/networks.py:82-112, train_ppo.py:121-126,136-139): z [B, A] = the MLP's last (linear) layer,
 *   mean = tanh(z), s = clip(log_std, -20, 2), act = mean + exp(s) eps, logp[B] = -0.5 sum((act -
 *   mean)^2 / exp(2 s) + 2 s + log 2 pi). Device pointers, float32, row-major. */
int mjl_obs_normalize(const float* x, const float* mean, const float* var, int n, int dim, float clip, float* y,
                      void* stream);
int mjl_policy_head(const float* z, const float* log_std, const float* eps, int B, int A, float* act, float* logp,
                    void* stream);

/* The rollout step's whole policy forward in one launch (train_ppo.py:134-139 with
 * src/networks.py:22-61,82-112: normalize_obs + clip, the GaussianPolicy MLP with tanh hidden
 * layers and a linear last layer, the tanh head, sampling and gaussian_logprob), on the matrix
 * cores: replaces mjl_obs_normalize + the MLP's GEMMs / activations + mjl_policy_head.
 * dims[0..nlayer] = obs_dim, hidden sizes..., act_dim (each <= 256, nlayer <= 6). params: per layer
 * WP[K/4][N][4] = W^T (K = in, N = out, both zero-padded to multiples of 16; WP[k/4][n][k%4] =
 * weight[n][k] of the torch / flax Dense) followed by the padded bias [N];
 * mjl_policy_param_floats(nlayer, dims) = its length. obs [B, obs_dim], eps [B, act_dim] -> act
 * [B, act_dim], logp [B]; device pointers, float32, row-major. */
long long mjl_policy_param_floats(int nlayer, const int* dims);
int mjl_policy_fwd(const float* obs, const float* mean, const float* var, float clip, const float* params, int nlayer,
                   const int* dims, const float* log_std, const float* eps, int B, float* act, float* logp,
                   void* stream);

/* APG with a stored forward instead of a recomputed one (train_apg.py:187-189 takes jax.grad with
 * per-step remat; HBM holds the forward instead): mjl_env_step_record is mjl_env_step without
 * auto-reset (same outputs and state update; derived fields are not stored) that also leaves in tape
 * slot `slot` what the step VJP's reverse passes read (workspace after integration, constraint rows,
 * the pre-step qpos / qvel / aux, the factor of the converged Hessian, the unrolled solve's tape);
 * mjl_env_step_vjp_replay is mjl_env_step_vjp_full of that step from the slot, without the
 * recompute and without restoring the pre-step state first. Requires MJL_OPT_VJP_TAPE; the VJP mode
 * (MJL_OPT_VJP_UNROLLED) must be the same at record and replay. On the humanoid dims the replay
 * (implicit, or unrolled with the CG solver) runs the lean layout: 19.5 KB of LDS per env, the dense
 * matrices read from the slot (environment MJL_VJP_LEAN=0 selects the full layout; same results). */
int mjl_env_step_record(mjlBatch* batch, int slot, const float* act, float* obs, float* rew, float* term,
                        float* trunc, void* stream);
/* mjl_env_step_record followed by mjl_apg_post's update of every env (below), as one launch where the
 * record keeps its rows in LDS (the implicit record on the humanoid dims), else the two launches. */
int mjl_env_step_record_apg(mjlBatch* batch, int slot, const float* act, float* obs, float* rew, float* term,
                            float* trunc, float gamma, float diverge_qvel, uint8_t* alive, float* disc, float* ret,
                            float* dropped, float* grew, float* rfin, void* stream);
/* 1 if mjl_env_step_record_apg_next applies to this batch (the implicit record on the humanoid dims). */
int mjl_env_record_fused(const mjlBatch* batch);
/* mjl_env_step_record_apg, then, from each env's new state and alive flag, mjl_apg_obs_policy_fwd's
 * observation (o, on, alive_snap) and small-MLP forward (ys) for the next rollout step, in the same
 * launch (the implicit record on the humanoid dims only: MJL_ERR_UNSUPPORTED otherwise). w_t[l]: layer
 * l's weight TRANSPOSED, [k_l, n_l] row-major; b[l], widths as mjl_small_mlp_fwd. */
int mjl_env_step_record_apg_next(mjlBatch* batch, int slot, const float* act, float* obs, float* rew, float* term,
                                 float* trunc, float gamma, float diverge_qvel, uint8_t* alive, float* disc, float* ret,
                                 float* dropped, float* grew, float* rfin, const float* mean, const float* var,
                                 int use_norm, float* o, float* on, uint8_t* alive_snap, int nl, const int* widths,
                                 const float* const* w_t, const float* const* b, float* const* ys, void* stream);
int mjl_env_step_vjp_replay(mjlBatch* batch, int slot, const float* act, const float* g_qpos, const float* g_qvel,
                            const float* g_qacc_ws, const float* g_rew, const float* g_aux, float* out_qpos,
                            float* out_qvel, float* out_qacc_ws, float* out_act, float* out_aux,
                            float* nonfinite_count, void* stream);
/* mjl_env_step_vjp_replay, then mjl_apg_policy_bwd_obs_vjp on its action cotangent, added to its state
 * cotangents before they are written (the same float operations), in one launch: w, widths, ys, o,
 * alive_snap, mean, var, use_norm as mjl_apg_policy_bwd_obs_vjp (the policy's output width = nu <= 32). */
int mjl_env_step_vjp_replay_apg(mjlBatch* batch, int slot, const float* act, const float* g_qpos,
                                const float* g_qvel, const float* g_qacc_ws, const float* g_rew, const float* g_aux,
                                float* out_qpos, float* out_qvel, float* out_qacc_ws, float* out_act, float* out_aux,
                                float* nonfinite_count, int nl, const int* widths, const float* const* w,
                                float* const* ys, const float* o, const uint8_t* alive_snap, const float* mean,
                                const float* var, int use_norm, void* stream);

/* APG rollout bookkeeping (train_apg.py:161-209; the sweep of mjx_amd/apg.py), one launch each per
 * rollout step. alive / alive_snap: uint8 [nenv] (0/1); device pointers, float32, row-major.
 * mjl_apg_obs: o [nenv, nq + nv] = [qpos | qvel] of each env (the APG observation); on = the policy
 *   input: x = alive ? o : 0, and with use_norm clip((x - mean) / (sqrt(var) + 1e-8), -10, 10)
 *   (train_apg.py:171-176); alive_snap = alive (for the backward).
 * mjl_apg_post: after the env step, per env: ok = rew, qpos, qvel finite (and max|qvel| <=
 *   diverge_qvel if > 0); bad = alive && !ok; dropped += bad; alive &= !bad; d = alive ? disc : 0;
 *   grew = -d / nenv (the reward's loss cotangent); ret += alive ? d rew : 0; rfin = rew if finite
 *   else 0; disc = d gamma (1 - max(term, trunc)); alive &= disc != 0.
 * mjl_apg_obs_vjp: g_qpos / g_qvel += (d on / d o)^T go at (o, alive_snap): zero where not alive,
 *   outside the clip, else go / (sqrt(var) + 1e-8) (go itself without use_norm). */
int mjl_apg_obs(mjlBatch* batch, const uint8_t* alive, const float* mean, const float* var, int use_norm, float* o,
                float* on, uint8_t* alive_snap, void* stream);
int mjl_apg_post(mjlBatch* batch, const float* rew, const float* term, const float* trunc, float gamma,
                 float diverge_qvel, uint8_t* alive, float* disc, float* ret, float* dropped, float* grew, float* rfin,
                 void* stream);
int mjl_apg_obs_vjp(int nenv, int nq, int nv, const float* o, const uint8_t* alive_snap, const float* mean,
                    const float* var, int use_norm, const float* go, float* g_qpos, float* g_qvel, void* stream);
/* The APG policy's per-step passes (src/networks.py:63-80 APGPolicy: Dense + tanh per layer, the
 * output tanh-squashed; train_apg.py:177 and its jax.grad): nl <= 4 layers, widths and k0 <= 64,
 * float32 row-major, w[l] = [widths[l], k_l] (torch Linear.weight), b[l] = [widths[l]], k_l = l ?
 * widths[l-1] : k0. mjl_small_mlp_fwd: ys[l] = tanh(ys[l-1] w[l]^T + b[l]) ([B, widths[l]], ys[-1] =
 * x), every sum in k order from the bias. mjl_small_mlp_bwd_input: g_x = d/dx of <g_out, ys[nl-1]>
 * from the forward's ys (the observation cotangent of the reverse sweep; no parameter gradients). */
int mjl_small_mlp_fwd(const float* x, int B, int k0, int nl, const int* widths, const float* const* w,
                      const float* const* b, float* const* ys, void* stream);
int mjl_small_mlp_bwd_input(const float* g_out, int B, int k0, int nl, const int* widths, const float* const* w,
                            const float* const* ys, float* g_x, void* stream);
/* The two fused per-step launches of the APG sweep (bit-identical to the pairs they replace):
 * mjl_apg_obs_policy_fwd = mjl_apg_obs, then mjl_small_mlp_fwd with x = on and k0 = nq + nv;
 * mjl_apg_policy_bwd_obs_vjp = mjl_small_mlp_bwd_input (k0 = nq + nv), then mjl_apg_obs_vjp with go = its
 * g_x (not stored). */
int mjl_apg_obs_policy_fwd(mjlBatch* batch, const uint8_t* alive, const float* mean, const float* var, int use_norm,
                           float* o, float* on, uint8_t* alive_snap, int nl, const int* widths, const float* const* w,
                           const float* const* b, float* const* ys, void* stream);
int mjl_apg_policy_bwd_obs_vjp(const float* g_out, int nenv, int nq, int nv, int nl, const int* widths,
                               const float* const* w, const float* const* ys, const float* o, const uint8_t* alive_snap,
                               const float* mean, const float* var, int use_norm, float* g_qpos, float* g_qvel,
                               void* stream);

/* PPO update (train_ppo.py:233-252, the bias-gradient column sums of every dense layer's backward
 * in value_and_grad of ppo_loss_fn / value_loss_fn, and the split-K weight-gradient sum):
 * out[d] = sum over rows of x[n, d] (row-major, float32, device), in a fixed order (two launches
 * when n > 256: per-chunk sums into `scratch`, then their sum). mjl_colsum_scratch(n, d) = the
 * scratch floats mjl_colsum needs (0: none, scratch may be NULL). */
long long mjl_colsum_scratch(int n, int d);
int mjl_colsum(const float* x, int n, int d, float* scratch, float* out, void* stream);
/* Backward of y = tanh(z) for a row-major [n, d] layer output (the PPO update's hidden layers; replaces
 * torch's tanh_backward + the bias gradient's column sum, src/networks.py:55-61 under jax.grad in
 * train_ppo.py:204-231): dz = g (1 - y^2), colsum_out[d] = dz.sum(0) in a fixed order (scratch: as
 * mjl_colsum). d % 4 == 0; g, y, dz, scratch and colsum_out 16-byte aligned. */
int mjl_tanh_bwd_colsum(const float* g, const float* y, int n, int d, float* dz, float* scratch, float* colsum_out,
                        void* stream);
/* out[e] = sum over s < ns of x[s * m + e] (slices summed in order: the split-K weight gradient's sum
 * over its batched GEMMs, in place of torch's sum(0)); m % 4 == 0, 16-byte aligned. */
int mjl_slice_sum(const float* x, int ns, long long m, float* out, void* stream);
/* x = tanh(x) elementwise in place (the update's hidden-layer activations, src/networks.py:55-61);
 * n % 4 == 0, 16-byte aligned. */
int mjl_tanh_inplace(float* x, long long n, void* stream);
/* The same reductions over nb stacked matrices (the twin update: the policy and value nets' layers
 * as one batched GEMM per layer, train_ppo.py:233-252 taking both nets' steps per minibatch):
 * x [nb][n][d] -> out [nb][d], each matrix summed in mjl_colsum's order; for nb > 1, n must be a
 * multiple of the 128-row chunk (n > 256). scratch: mjl_colsum_batched_scratch(nb, n, d) floats.
 * mjl_slice_sum_batched: out[b][e] = sum over s < ns of x[(b * ns + s) * m + e]. */
long long mjl_colsum_batched_scratch(int nb, int n, int d);
/* The first stage alone, with the caller's row chunk: dz = g (1 - y^2) written out and partials
 * [nb][n / chunk][d] = each chunk's column sums of dz, for mjl_slice_sum_multi to finish.
 * n % chunk == 0, d % 4 == 0, 16-byte aligned buffers. */
int mjl_tanh_bwd_colsum_partials(const float* g, const float* y, int nb, int n, int d, int chunk, float* dz,
                                 float* partials, void* stream);
int mjl_colsum_batched(const float* x, int nb, int n, int d, float* scratch, float* out, void* stream);
int mjl_tanh_bwd_colsum_batched(const float* g, const float* y, int nb, int n, int d, float* dz, float* scratch,
                                float* colsum_out, void* stream);
int mjl_slice_sum_batched(const float* x, int nb, int ns, long long m, float* out, void* stream);
/* nseg <= 16 slice sums in one launch: out_k[b][e] = sum over s < ns[k] (in order) of
 * x_k[(b * ns[k] + s) * m[k] + e], b < nb[k] (the twin update's weight-gradient slices and column-sum
 * partials of every layer, reduced together at the end of its backward). step0 / step1 / ctr (device
 * float / float / int, each or NULL) are advanced by one in the same launch: the captured update's
 * step counters and minibatch row, after their last read in the step (mjl_adam_multi then runs with
 * advanced = 1). */
int mjl_slice_sum_multi(int nseg, const float* const* x, float* const* out, const int* nb, const int* ns,
                        const long long* m, float* step0, float* step1, int* ctr, void* stream);
/* The twin update's losses and output-layer backward in one pass (train_ppo.py:204-220 for both nets):
 * z [2][n][A], z[0] = the policy's mean (tanh of its last Dense, networks.py:103), z[1][:, 0] = the
 * value (the value net's output layer padded to A rows); the clipped surrogate as
 * mjl_ppo_surrogate_clipped (advantages normalised by adv_stats — a [n_minibatches, 2] table read at
 * *stats_row when stats_row is given — or over the n rows when adv_stats is NULL), the value loss
 * mean (v - ret)^2 (train_ppo.py:218-220). Writes dz [2][n][A]: dz[0] = d loss / d mean (1 - mean^2),
 * dz[1][:, 0] = 2 (v - ret) / n, dz[1][:, 1:] = 0; and per block b < mjl_twin_loss_head_blocks(n) the
 * partials whose in-order sums over b (mjl_slice_sum_multi) are the results: lossp [nb] -> the policy
 * loss, glsp [nb][A] -> d loss / d log_std (clip mask included), biasp [2][nb][A] -> both output
 * biases' gradients. bias (or NULL): z holds the output layers' pre-activations and bias [2][A] their
 * biases — mean = tanh(z[0] + bias[0]), v = z[1][:, 0] + bias[1][0]. scratch: mjl_ppo_loss_scratch(n, A)
 * floats. A <= 32. */
long long mjl_twin_loss_head_blocks(int n);

/* The twin PPO update's thin ends as single launches (train_ppo.py:233-252 run_ppo_updates over the
   src/networks.py:82-131 MLPs; both nets stacked as in mjl_twin_loss_head). Bit 0 of
   mjl_twin_fused_shapes: mjl_twin_gather_in is instantiated for (k0, N); bit 1: mjl_twin_head_bwd for
   (A, N). Other shapes take the library GEMM path. */
int mjl_twin_fused_shapes(int k0, int A, int N);
/* The minibatch gather (make_index_batches' rows, train_ppo.py:222-231; idx [n], or row *idx_row of an
   [n_minibatches, n] table) fused with both nets' input layer: o2 [2, n, k0] (the observations twice),
   a [n, A], ol / r / ad [n] gathered from obs / act / logp / ret / adv (an out-of-range index gives NaN);
   h [2, n, N] = tanh(o W[net]^T + b[net]) with W [2, N, k0], b [2, N]. */
int mjl_twin_gather_in(const long long* idx, const int* idx_row, int n, long long nsrc, int k0, int A, int N,
                       const float* obs, const float* act, const float* logp, const float* ret, const float* adv,
                       float* o2, float* a, float* ol, float* r, float* ad, const float* W, const float* b,
                       float* h, void* stream);
/* The output layers' backward fused with the last hidden layer's tanh backward: dzh [2, n, N] =
   (dz W) (1 - y^2) for dz [2, n, A], W [2, A, N], y [2, n, N]; per chunk c of 128 rows the column sums of
   dzh into cs [2, n/128, N] and the output weight gradient's partial dz^T y into gw [2, n/128, A, N]
   (summed by mjl_slice_sum_multi). n % 128 == 0, 16-byte aligned buffers. */
int mjl_twin_head_bwd(const float* dz, const float* W, const float* y, int n, int A, int N, float* dzh, float* cs,
                      float* gw, void* stream);
/* The twin update's whole head in one launch (bit 2 of mjl_twin_fused_shapes; train_ppo.py:204-220 on
   both nets' output layers): H = tanh(zh + bh) for the last hidden layer's bias-less GEMM output zh
   [2, n, K] and bias bh [2, K]; z = H W^T + bo (W [2, A, K], bo [2, A]); the policy's clipped
   surrogate + entropy and the value's MSE gradient exactly as mjl_twin_loss_head (advantages
   normalised by row *stats_row of adv_stats, or, adv_stats NULL, by this minibatch's own statistics
   through scratch of mjl_ppo_loss_scratch(n, A) floats); then dzh [2, n, K] = (dz W)(1 - H^2). Per
   workgroup b < S = mjl_twin_head_blocks(n) of each net k, partials summed in order by
   mjl_slice_sum_multi: lossp[b] (policy loss, b = 0 adds the entropy term), glsp[b][A] (log_std),
   biasp[k][b][A] (output biases), cs[k][b][K] (the last hidden bias), gw[k][b][A][K] (output weights).
   n % 64 == 0. */
long long mjl_twin_head_blocks(int n);
int mjl_twin_head(const float* zh, const float* bh, const float* W, const float* bo, const float* log_std,
                  const float* act, const float* old_logp, const float* adv, const float* ret, const float* adv_stats,
                  const int* stats_row, int n, int A, int K, float clip_eps, float ent_coef, float log_std_lo,
                  float log_std_hi, float* scratch, float* dzh, float* cs, float* gw, float* lossp, float* glsp,
                  float* biasp, void* stream);
int mjl_twin_loss_head(const float* z, const float* log_std, const float* act, const float* old_logp, const float* adv,
                       const float* ret, const float* adv_stats, const int* stats_row, int n, int A, float clip_eps,
                       float ent_coef, float log_std_lo, float log_std_hi, const float* bias, float* scratch,
                       float* dz, float* lossp, float* glsp, float* biasp, void* stream);
/* x[b][r][j] = act_b(x[b][r][j] + bias[b][j]) in place over nb stacked row-major [rows, n] matrices,
 * act_b = tanh when bit b of act_mask is set, else the identity (the twin update's dense-layer
 * epilogue, src/networks.py:55-61, after a bias-less batched GEMM). */
int mjl_bias_act(float* x, const float* bias, int nb, long long rows, int n, unsigned act_mask, void* stream);

/* PPO update losses (train_ppo.py:204-220), forward and gradient in one pass, deterministic.
 * mjl_ppo_surrogate: loss = -mean_i min(r_i an_i, clip(r_i, 1 - clip_eps, 1 + clip_eps) an_i)
 *   - ent_coef 0.5 sum_j (1 + log 2 pi + 2 log_std_j) / A, with r_i = exp(logp_i - old_logp_i),
 *   logp the diagonal Gaussian log-density of act under (mean, exp(log_std)) and an the advantage
 *   normalised over the n rows, (adv - mean) / (population std + 1e-8) — or by adv_stats = (mean,
 *   std) when given (device, the data-parallel minibatch's global statistics); g_mean [n, A] and
 *   g_log_std [A] are d loss / d mean and d loss / d log_std (torch.minimum / clamp conventions for
 *   ties and bounds). mjl_mse: loss = mean (v - r)^2, g_v = 2 (v - r) / n. scratch:
 *   mjl_ppo_loss_scratch(n, A) floats (mjl_mse needs n / 256 + 1). A <= 32.
 * mjl_gather_rows: dst_k[r, :] = src_k[idx[r], :] for narr <= 8 row-major float arrays of nsrc rows
 *   and cols[k] columns (the minibatch gather of train_ppo.py:237-241), idx int64 [n]; one launch;
 *   an index outside [0, nsrc) gives a NaN row; n x (total columns) must be below 2^31. */
long long mjl_ppo_loss_scratch(int n, int A);
int mjl_ppo_surrogate(const float* mean, const float* log_std, const float* act, const float* old_logp,
                      const float* adv, const float* adv_stats, int n, int A, float clip_eps, float ent_coef,
                      float* scratch, float* loss, float* g_mean, float* g_log_std, void* stream);
int mjl_mse(const float* v, const float* r, int n, float* scratch, float* loss, float* g_v, void* stream);
/* mjl_ppo_surrogate with log_std clipped to [log_std_lo, log_std_hi] on read (networks.py:103 clips it
 * to [-20, 2]) and g_log_std zero where the raw value lies outside (torch.clamp's backward, bounds
 * inclusive); +-INFINITY bounds = mjl_ppo_surrogate. stats_row (device int, or NULL): adv_stats is an
 * [n_minibatches, 2] table read at that row (a captured minibatch step reads its row at run time). */
int mjl_ppo_surrogate_clipped(const float* mean, const float* log_std, const float* act, const float* old_logp,
                              const float* adv, const float* adv_stats, const int* stats_row, int n, int A,
                              float clip_eps, float ent_coef, float log_std_lo, float log_std_hi, float* scratch,
                              float* loss, float* g_mean, float* g_log_std, void* stream);
/* mjl_mse with v[i] read at v + i * vstride (the value column of the twin update's padded output). */
int mjl_mse_strided(const float* v, int vstride, const float* r, int n, float* scratch, float* loss, float* g_v,
                    void* stream);
int mjl_gather_rows(const long long* idx, int n, long long nsrc, int narr, const float* const* src, float* const* dst,
                    const int* cols, void* stream);
/* mjl_gather_rows from row *idx_row (device int) of an [n_minibatches, n] index table (NULL: idx). */
int mjl_gather_rows_indexed(const long long* idx, const int* idx_row, int n, long long nsrc, int narr,
                            const float* const* src, float* const* dst, const int* cols, void* stream);
/* Adam (optax.adam defaults as train_ppo.py:84-85 build them; torch.optim.Adam's fused update) over
 * nt <= 16 float32 tensors in one launch: m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
 * p -= lr / (1 - b1^step) m / (sqrt(v) / sqrt(1 - b2^step) + eps); g[k] NULL skips tensor k. */
int mjl_adam(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
             const long long* numel, float lr, float beta1, float beta2, float eps, int step, void* stream);
/* mjl_adam with the step count read from device memory at execution time (step: device float, the
 * step being taken, >= 1), so a hipGraph that captured the call takes the bias corrections of each
 * replay's own step (the caller's captured increment advances it; train_ppo.py:233-252 runs the whole
 * update as one compiled scan, optax keeping the count as device state). */
int mjl_adam_dev(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                 const long long* numel, float lr, float beta1, float beta2, float eps, const float* step,
                 void* stream);

/* Adam over nt <= 24 tensors of up to 2 optimisers in one launch (the PPO update's policy and value
 * steps, train_ppo.py:246-251): tensor k uses group[k]'s lr and device step counter step[group[k]]
 * (float, the count before this step: the step takes step + 1, and every group's counter is advanced
 * by one after it); g is scaled by gscale (the data-parallel mean: 1 / world size); ctr (device int,
 * or NULL) is advanced with the counters. advanced = 1: the counters were advanced earlier in the
 * minibatch step (mjl_slice_sum_multi's step0 / step1 / ctr): the step takes step as it is and
 * nothing is advanced here. Same arithmetic as mjl_adam_dev. */
int mjl_adam_multi(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                   const long long* numel, const int* group, int ngroups, const float* lr, float beta1, float beta2,
                   float eps, float gscale, float* const* step, int* ctr, int advanced, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Batched ray-cast renderer: RGB / depth / segmentation frames from qpos. Replaces the
 * mujoco.Renderer loop of src/rendering.py:181-192 (mj_forward + update_scene + render per frame)
 * and serves per-env camera images of a batch. Planes, spheres and capsules have closed-form ray
 * intersections, so there is no GL and no mesh pipeline; the shading model is DESIGN.md "Rendering".
 *
 * mjlVisualDesc is what the MJCF compiler keeps beside mjlModelDesc (mjx_amd/mjcf.py, `visual`):
 *   geom_rgba               per-geom colour (alpha is carried, not rendered)
 *   checker_*               the plane geom with a builtin checker texture (checker_geom, -1 = none): its two
 *                           colours, the world-space cell size along the plane's x / y, and those two axes in
 *                           the frame of the geom's body
 *   sky_rgb1 / sky_rgb2     a miss takes (1 - s) rgb2 + s rgb1 with s = (1 + d_z) / 2 of the ray direction d
 *   light_*                 the one light, frozen in the world at qpos0: position, or direction when
 *                           light_directional; diffuse colour; ambient term
 *   znear, zfar             hits are kept for ray parameters in [znear, zfar] (metres)
 *   cam_*                   ncam <= MJL_MAXCAM cameras: body, MJL_CAM_* mode (any other value: the camera
 *                           cannot be selected), vertical field of view in degrees; cam_pos / cam_mat the pose in
 *                           the body's frame (fixed cameras); cam_pos0 / cam_mat0 the world offset from the body's
 *                           position (track) or subtree centre of mass (trackcom) and the world rotation, both
 *                           at qpos0 (MuJoCo's cam_pos0 / cam_poscom0 / cam_mat0). Rotations are row-major with
 *                           the camera's x (right), y (up), z axes as columns; the camera looks along -z.
 * ------------------------------------------------------------------------------------------- */
#define MJL_MAXCAM 8
enum { MJL_CAM_FIXED = 0, MJL_CAM_TRACK = 1, MJL_CAM_TRACKCOM = 2 };
enum { MJL_RENDER_SHADOWS = 1 };

typedef struct mjlVisualDesc {
  int32_t ncam, checker_geom, light_directional;
  float geom_rgba[MJL_MAXGEOM][4];
  float checker_rgb1[3], checker_rgb2[3], checker_cell[2], checker_xaxis[3], checker_yaxis[3];
  float sky_rgb1[3], sky_rgb2[3];
  float light_pos[3], light_dir[3], light_diffuse[3], light_ambient[3];
  float znear, zfar;
  int32_t cam_body[MJL_MAXCAM], cam_mode[MJL_MAXCAM];
  float cam_fovy[MJL_MAXCAM];
  float cam_pos[MJL_MAXCAM][3], cam_mat[MJL_MAXCAM][9], cam_pos0[MJL_MAXCAM][3], cam_mat0[MJL_MAXCAM][9];
} mjlVisualDesc;

typedef struct mjlRenderer mjlRenderer;

/* A renderer for `model` on `device`: uploads the model and visual constants and allocates the
 * per-frame scene scratch for up to max_frames (1..65535) frames per call. MJL_ERR_UNSUPPORTED for a
 * geom type other than plane, sphere or capsule. The model may be destroyed afterwards. */
int mjl_renderer_create(const mjlModel* model, const mjlVisualDesc* visual, int max_frames, int device,
                        mjlRenderer** out);
void mjl_renderer_destroy(mjlRenderer* renderer);
/* Render n <= max_frames frames through camera `camera` at width x height pixels, two launches on
 * `stream`, no allocation and no synchronisation. qpos: device float32 [n, nq] (any buffer: a qpos
 * history, or a batch's MJL_FIELD_QPOS rows); forward kinematics only, no batch and no constraint
 * solve. rgb uint8 [n, height, width, 3]; depth float32 [n, height, width], the distance along the
 * pixel's ray, +inf where nothing lies within zfar; seg int32 [n, height, width], the geom id, -1 =
 * background. Each output may be NULL, not all three. flags: MJL_RENDER_SHADOWS adds hard shadows.
 * MJL_ERR_ARG for n > max_frames, a non-positive size, a camera outside the visual description's
 * cameras or all outputs NULL; MJL_ERR_UNSUPPORTED for a camera whose mode is not an MJL_CAM_* one. */
int mjl_render_qpos(mjlRenderer* renderer, const float* qpos, int n, int camera, int width, int height, int flags,
                    uint8_t* rgb, float* depth, int32_t* seg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MJX355_H_ */
