// mjx355 C ABI (include/mjx355.h): model upload, batch state ownership, kernel launches.
// Host side only; the kernels live in step_kernels.hip (same translation unit), the conversion of a model
// descriptor into the device's model block in model_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>

#include "step_kernels.hip"
#include "substep_kernels.hip"
#include "adjoint.hip"
#include "ppo_kernels.hip"
#include "apg_kernels.hip"
#include "ppo_loss_kernels.hip"
#include "twin_kernels.hip"
#include "render_kernels.hip"
#include "contact_kernels.hip"
#include "sensor_kernels.hip"
#include "body_kernels.hip"
#include "dyn_kernels.hip"
#include "ik_kernels.hip"
#include "taskspace_kernels.hip"
#include "inverse_kernels.hip"
#include "linearize_kernels.hip"
#include "ray_kernels.hip"
#include "distance_kernels.hip"
#include "model_host.h"

using namespace mjl;

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) return fail(MJL_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

}  // namespace

struct mjlModel {
  mjlModelDesc desc;
  ModelF mf;
  SensorTab st;  // the readout table of mjl_sensors (st.n = 0: the model has none)
  BodyTab bt;    // body_iquat, for mjl_body_data's ximat
  DynTab dt;     // body_dofmask, for mjl_jac's columns
  int nefc_max, ncon_max, nvc;  // nvc: 0 = DHum kernels, 1 = DGen kernels
};

// One env's VJP tape slot, in floats: the workspace image at w, the A part (SlotA) at a, the global row
// slab at r, the unrolled solve's tape at t; each section starts on a multiple of 4 floats.
struct TapeLayout { int w, a, r, t; long long stride; };
static TapeLayout tape_layout(bool gen, int gmax_efc, int gmax_con, int iterations) {
  // (the workspace image needs no rounding: the parenthesisation below rounds an already whole value)
  static_assert(slot_w_floats<DGen>() % 4 == 0 && slot_w_floats<DHumV>() % 4 == 0, "WS is a whole number of b128");
  const int LD = gen ? DGen::LD : DHumV::LD;
  TapeDims td;
  td.init(LD, gmax_efc, iterations);
  const long long r4 = 3;
  TapeLayout L;
  L.w = 0;
  L.a = (int)((gen ? slot_w_floats<DGen>() : slot_w_floats<DHumV>()) + r4) & ~3;
  L.r = (int)((L.a + (gen ? slot_a_floats<DGen>() : slot_a_floats<DHumV>()) + r4) & ~3);
  L.t = (int)(L.r + (((long long)row_slab_floats(LD, gmax_efc, gmax_con) + r4) & ~r4));
  L.stride = ((long long)L.t + td.tape + r4) & ~r4;
  return L;
}

struct mjlBatch {
  const mjlModel* model;
  int device, nenv, store_derived, force_global_rows;
  int simds;  // SIMDs of the device (4 per CU): the largest launch that is one wave per SIMD
  ModelF* d_model;
  mjlEnvConfig* d_env;
  int has_env, obs_dim;
  float* d_state;  // one slab holding every per-env field
  StateBuf s;
  int dim[MJL_NFIELD];
  float* field_ptr[MJL_NFIELD];
  float* d_scratch;
  int scratch_stride, gmax_efc, gmax_con;
  float* d_adj_scratch;  // step VJP: per env row slab + adjoint scratch (allocated on first use)
  int vjp_unrolled;      // MJL_OPT_VJP_UNROLLED
  float* d_unr;          // unrolled VJP: per env solve tape + row accumulators (allocated on first use)
  TapeDims unr_dims;
  int adj_stride, adj_row_floats;
  int adj_blocks;        // strides d_adj_scratch holds: nenv, or nenv x row groups once mjl_step_jacobian has run
  int lin_groups;        // MJL_OPT_LINEARIZE_GROUPS: row groups per env of mjl_step_jacobian, 0 = the host's rule
  const unsigned long long* ctr_base;  // device RNG counter base (mjl_batch_set_counter_base), or null
  int* vjp_exp;       // per-env cotangent exponents of the guarded env-step VJPs (mjl_vjp_scale_attach), or null
  int vjp_exp_thr;    // log2 of the output magnitude from which an env's cotangents are rescaled
  float* d_exp_stage; // per env kExpStage floats: rescaled input cotangents (allocated by the first attach)
  const uint32_t* reset_keys;           // per-env jax.random reset keys (mjl_env_set_reset_keys), or null
  int key_mode;
  float* d_vtape;  // MJL_OPT_VJP_TAPE: slots x nenv x vtape_stride floats (record / replay), or null
  int vtape_slots;
  TapeLayout vt;
  float* d_rs;     // MJL_OPT_RESET_POOL: pool slots (the state fields again, [slots * nenv] rows) + obs
  int* d_pool_ctl;  // [nenv, 2] next slot, filled slots
  int pool_slots;
  StateBuf rs;
  float* rs_obs;
  const float* qfrc_applied;  // caller-owned applied forces (mjl_batch_attach_applied), or null
  const float* xfrc_applied;
  ModelF* d_model_env;      // MJL_OPT_PER_ENV_MODEL: one model block per env, or null
  ParamStage* d_param_stage;  // what model_params_kernel needs beside the blocks (allocated with them)
  SensorTab* d_sensors;       // the readout table beside the model block, or null (a model without readout sensors)
  BodyTab* d_bodytab;         // body_iquat beside the model block (mjl_body_data)
  DynTab* d_dyntab;           // body_dofmask beside the model block (mjl_jac)
  int ray_chunk;              // MJL_OPT_RAY_CHUNK: rays per wavefront of mjl_ray / mjl_ray_scan, 0 = kRayChunk
  int dist_chunk;             // MJL_OPT_DISTANCE_CHUNK: pairs per wavefront of mjl_geom_distance, 0 = kDistChunk
};

// one launch of the per-env block builder: `fill` copies the shared block into every env's
static int launch_model_params(mjlBatch* B, const float* const* values, const float* mask, int fill, void* stream) {
  ModelParamArgs A;
  A.nominal = B->d_model; A.blocks = B->d_model_env; A.stage = B->d_param_stage;
  for (int k = 0; k < MJL_NMP; k++) A.v[k] = values ? values[k] : nullptr;
  A.mask = mask; A.nenv = B->nenv; A.fill = fill;
  hipLaunchKernelGGL(model_params_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// Row groups per env of mjl_step_jacobian (linearize_kernels.hip): each group's wave repeats the step's forward
// and sweeps its share of the output rows. The most the host rule picks and MJL_OPT_LINEARIZE_GROUPS accepts.
constexpr int kLinMaxGroups = 16;

extern "C" {

const char* mjl_last_error(void) { return g_err.c_str(); }
#ifndef MJL_SRC_HASH
#define MJL_SRC_HASH "unstamped"
#endif
// "mjx355 <ver> (gfx950) src=<hash>": the hash of the sources this library was built from
// (mjx_amd/_srchash.py, stamped by the Makefile); the loader refuses a stale library
const char* mjl_version(void) { return "mjx355 0.2 (gfx950) src=" MJL_SRC_HASH; }

#ifdef MJL_TIMING
// diagnostic build only: install a device buffer [nenv, 16] of per-phase s_memtime stamps
int mjl_debug_set_stamps(unsigned long long* dev_buf) {
  HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(mjl::g_stamps), &dev_buf, sizeof(dev_buf)));
  return MJL_OK;
}
#endif

int mjl_model_create(const mjlModelDesc* d, mjlModel** out) {
  if (!d || !out) return fail(MJL_ERR_ARG, "null argument");
  *out = nullptr;
  std::unique_ptr<mjlModel> M(new (std::nothrow) mjlModel());
  if (!M) return fail(MJL_ERR_ARG, "out of host memory");
  std::string msg;
  if (int rc = model_build(d, M->mf, M->nefc_max, M->ncon_max, msg)) return fail(rc, "%s", msg.c_str());
  M->desc = *d;
  sensor_tab_build(d, M->st);
  body_tab_build(d, M->bt);
  dyn_tab_build(d, M->dt);
  // compact kernel instantiation when the model fits the humanoid capacities, generic otherwise
  M->nvc = (d->nv <= DHum::NV && d->nbody <= DHum::NB && d->njnt <= DHum::NJ && d->ngeom <= DHum::NG) ? 0 : 1;
  *out = M.release();
  return MJL_OK;
}

void mjl_model_destroy(mjlModel* m) { delete m; }
int mjl_model_nefc_max(const mjlModel* m) { return m ? m->nefc_max : -1; }
int mjl_model_ncon_max(const mjlModel* m) { return m ? m->ncon_max : -1; }
int mjl_model_nrsensordata(const mjlModel* m) { return m ? m->st.ndata : -1; }

int mjl_batch_create(const mjlModel* model, int nenv, int device, mjlBatch** out) {
  if (!model || !out || nenv <= 0) return fail(MJL_ERR_ARG, "bad argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MJL_ERR_NOGPU, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(MJL_ERR_ARG, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));
  mjlBatch* B = new (std::nothrow) mjlBatch();
  if (!B) return fail(MJL_ERR_ARG, "out of host memory");
  std::memset(B, 0, sizeof(*B));
  B->model = model; B->device = device; B->nenv = nenv; B->store_derived = 1;
  {
    int ncu = 0;
    if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) ncu = 0;
    B->simds = 4 * ncu;
  }
  const mjlModelDesc& d = model->desc;
  int* dim = B->dim;
  dim[MJL_FIELD_QPOS] = d.nq; dim[MJL_FIELD_QVEL] = d.nv; dim[MJL_FIELD_QACC_WARMSTART] = d.nv;
  dim[MJL_FIELD_TIME] = 1; dim[MJL_FIELD_CTRL] = d.nu; dim[MJL_FIELD_QACC] = d.nv;
  dim[MJL_FIELD_XPOS] = d.nbody * 3; dim[MJL_FIELD_XQUAT] = d.nbody * 4; dim[MJL_FIELD_QFRC_ACTUATOR] = d.nv;
  dim[MJL_FIELD_SENSORDATA] = d.nsensordata > 0 ? d.nsensordata : 1; dim[MJL_FIELD_AUX] = MJL_AUX_DIM;
  dim[MJL_FIELD_STATS] = 4; dim[MJL_FIELD_QFRC_BIAS] = d.nv; dim[MJL_FIELD_QFRC_PASSIVE] = d.nv;
  dim[MJL_FIELD_QFRC_CONSTRAINT] = d.nv; dim[MJL_FIELD_QACC_SMOOTH] = d.nv;
  size_t total = 0;
  for (int f = 0; f < MJL_NFIELD; f++) total += (size_t)dim[f] * nenv;
  hipError_t e = hipMalloc(&B->d_state, total * sizeof(float));
  if (e != hipSuccess) { delete B; return fail(MJL_ERR_HIP, "hipMalloc state: %s", hipGetErrorString(e)); }
  size_t off = 0;
  for (int f = 0; f < MJL_NFIELD; f++) { B->field_ptr[f] = B->d_state + off; off += (size_t)dim[f] * nenv; }
  StateBuf& s = B->s;
  for (int f = 0; f < MJL_NFIELD; f++) s.*kStateField[f] = B->field_ptr[f];
  // make_data: zeros, qpos = qpos0
  e = hipMemset(B->d_state, 0, total * sizeof(float));
  if (e == hipSuccess) {
    float* q = new float[(size_t)d.nq * nenv];
    for (int i = 0; i < nenv; i++)
      for (int k = 0; k < d.nq; k++) q[(size_t)i * d.nq + k] = (float)d.qpos0[k];
    e = hipMemcpy(s.qpos, q, sizeof(float) * d.nq * nenv, hipMemcpyHostToDevice);
    delete[] q;
  }
  if (e == hipSuccess) e = hipMalloc(&B->d_model, sizeof(ModelF));
  if (e == hipSuccess) e = hipMemcpy(B->d_model, &model->mf, sizeof(ModelF), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&B->d_env, sizeof(mjlEnvConfig));
  if (e == hipSuccess && model->st.n > 0) {
    e = hipMalloc(&B->d_sensors, sizeof(SensorTab));
    if (e == hipSuccess) e = hipMemcpy(B->d_sensors, &model->st, sizeof(SensorTab), hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMalloc(&B->d_bodytab, sizeof(BodyTab));
  if (e == hipSuccess) e = hipMemcpy(B->d_bodytab, &model->bt, sizeof(BodyTab), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&B->d_dyntab, sizeof(DynTab));
  if (e == hipSuccess) e = hipMemcpy(B->d_dyntab, &model->dt, sizeof(DynTab), hipMemcpyHostToDevice);
  // global overflow rows for envs whose active constraints exceed the LDS capacity
  int LD = model->nvc == 0 ? DHum::LD : DGen::LD;
  B->gmax_efc = model->nefc_max > 0 ? model->nefc_max : 1;
  B->gmax_con = model->ncon_max > 0 ? model->ncon_max : 1;
  B->scratch_stride = row_slab_floats(LD, B->gmax_efc, B->gmax_con);
  B->scratch_stride = (B->scratch_stride + 3) & ~3;
  if (e == hipSuccess) e = hipMalloc(&B->d_scratch, (size_t)B->scratch_stride * nenv * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(B->d_state); (void)hipFree(B->d_model); (void)hipFree(B->d_env); (void)hipFree(B->d_scratch);
    (void)hipFree(B->d_sensors); (void)hipFree(B->d_bodytab); (void)hipFree(B->d_dyntab);
    delete B;
    return fail(MJL_ERR_HIP, "batch allocation: %s", hipGetErrorString(e));
  }
  *out = B;
  return MJL_OK;
}

void mjl_batch_destroy(mjlBatch* B) {
  if (!B) return;
  (void)hipSetDevice(B->device);
  (void)hipFree(B->d_state); (void)hipFree(B->d_model); (void)hipFree(B->d_env); (void)hipFree(B->d_scratch);
  (void)hipFree(B->d_adj_scratch);
  (void)hipFree(B->d_unr);
  (void)hipFree(B->d_exp_stage);
  (void)hipFree(B->d_rs); (void)hipFree(B->d_pool_ctl); (void)hipFree(B->d_vtape);
  (void)hipFree(B->d_model_env); (void)hipFree(B->d_param_stage);
  (void)hipFree(B->d_sensors); (void)hipFree(B->d_bodytab); (void)hipFree(B->d_dyntab);
  delete B;
}

int mjl_batch_nenv(const mjlBatch* B) { return B ? B->nenv : -1; }

int mjl_batch_set_option(mjlBatch* B, int option, int value) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (option == MJL_OPT_STORE_DERIVED) { B->store_derived = value != 0; return MJL_OK; }
  if (option == MJL_OPT_FORCE_GLOBAL_ROWS) { B->force_global_rows = value != 0; return MJL_OK; }
  if (option == MJL_OPT_VJP_UNROLLED) {
    if (value && B->model->desc.iterations > 256)
      return fail(MJL_ERR_ARG, "unrolled VJP: %d solver iterations (at most 256 are taped)", B->model->desc.iterations);
    // a zoom line search creates up to 1 + 2 ls_iterations Newton points; the tape holds 64 per search
    if (value && 1 + 2 * B->model->desc.ls_iterations > 64)
      return fail(MJL_ERR_ARG, "unrolled VJP: ls_iterations %d (at most 31: the tape holds 64 line-search points)",
                  B->model->desc.ls_iterations);
    B->vjp_unrolled = value != 0;
    return MJL_OK;
  }
  if (option == MJL_OPT_VJP_TAPE) {
    if (value < 0) return fail(MJL_ERR_ARG, "VJP tape: slots must be >= 0");
    HIPCHK(hipSetDevice(B->device));
    (void)hipFree(B->d_vtape);
    B->d_vtape = nullptr; B->vtape_slots = 0;
    if (!value) return MJL_OK;
    B->vt = tape_layout(B->model->nvc != 0, B->gmax_efc, B->gmax_con, B->model->desc.iterations);
    const size_t bytes = (size_t)value * B->nenv * (size_t)B->vt.stride * sizeof(float);
    hipError_t e = hipMalloc(&B->d_vtape, bytes);
    if (e != hipSuccess) { B->d_vtape = nullptr; return fail(MJL_ERR_HIP, "VJP tape (%zu bytes): %s", bytes, hipGetErrorString(e)); }
    B->vtape_slots = value;
    return MJL_OK;
  }
  if (option == MJL_OPT_RESET_POOL) {
    if (value < 0 || value > 64) return fail(MJL_ERR_ARG, "reset pool: 0..64 slots per env");
    HIPCHK(hipSetDevice(B->device));
    (void)hipFree(B->d_rs); (void)hipFree(B->d_pool_ctl);
    B->d_rs = nullptr; B->d_pool_ctl = nullptr; B->pool_slots = 0;
    if (!value) return MJL_OK;
    const size_t rows = (size_t)value * B->nenv;
    size_t total = 0;
    for (int f = 0; f < MJL_NFIELD; f++) total += (size_t)B->dim[f] * rows;
    const size_t obs_floats = (size_t)64 * rows;  // obs_dim <= 64 (mjl_env_config)
    hipError_t e = hipMalloc(&B->d_rs, (total + obs_floats) * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&B->d_pool_ctl, (size_t)B->nenv * 2 * sizeof(int));
    if (e == hipSuccess) e = hipMemset(B->d_pool_ctl, 0, (size_t)B->nenv * 2 * sizeof(int));  // empty
    if (e != hipSuccess) {
      (void)hipFree(B->d_rs); (void)hipFree(B->d_pool_ctl);
      B->d_rs = nullptr; B->d_pool_ctl = nullptr;
      return fail(MJL_ERR_HIP, "reset pool: %s", hipGetErrorString(e));
    }
    size_t off = 0;
    for (int k = 0; k < MJL_NFIELD; k++) { B->rs.*kStateField[k] = B->d_rs + off; off += (size_t)B->dim[k] * rows; }
    B->rs_obs = B->d_rs + total;
    B->pool_slots = value;
    return MJL_OK;
  }
  if (option == MJL_OPT_PER_ENV_MODEL) {
    HIPCHK(hipSetDevice(B->device));
    (void)hipFree(B->d_model_env); (void)hipFree(B->d_param_stage);
    B->d_model_env = nullptr; B->d_param_stage = nullptr;
    if (!value) return MJL_OK;
    const size_t bytes = (size_t)B->nenv * sizeof(ModelF);
    ParamStage st;
    model_param_stage(&B->model->desc, st);
    hipError_t e = hipMalloc(&B->d_model_env, bytes);
    if (e == hipSuccess) e = hipMalloc(&B->d_param_stage, sizeof(ParamStage));
    if (e == hipSuccess) e = hipMemcpy(B->d_param_stage, &st, sizeof(ParamStage), hipMemcpyHostToDevice);
    int rc = MJL_OK;
    if (e == hipSuccess) {
      rc = launch_model_params(B, nullptr, nullptr, 1, nullptr);
      if (rc == MJL_OK) e = hipStreamSynchronize(nullptr);
    }
    if (e != hipSuccess || rc != MJL_OK) {
      (void)hipFree(B->d_model_env); (void)hipFree(B->d_param_stage);
      B->d_model_env = nullptr; B->d_param_stage = nullptr;
      return e != hipSuccess ? fail(MJL_ERR_HIP, "per-env model blocks (%zu bytes): %s", bytes, hipGetErrorString(e)) : rc;
    }
    return MJL_OK;
  }
  if (option == MJL_OPT_RAY_CHUNK) {
    if (value < 0 || value > 65535) return fail(MJL_ERR_ARG, "ray chunk: 0..65535 rays per wavefront");
    B->ray_chunk = value;
    return MJL_OK;
  }
  if (option == MJL_OPT_DISTANCE_CHUNK) {
    if (value < 0 || value > 65535) return fail(MJL_ERR_ARG, "distance chunk: 0..65535 pairs per wavefront");
    B->dist_chunk = value;
    return MJL_OK;
  }
  if (option == MJL_OPT_LINEARIZE_GROUPS) {
    if (value < 0 || value > kLinMaxGroups)
      return fail(MJL_ERR_ARG, "linearize groups: 0..%d row groups per env", kLinMaxGroups);
    B->lin_groups = value;
    return MJL_OK;
  }
  return fail(MJL_ERR_ARG, "unknown option %d", option);
}

int mjl_model_param_dim(const mjlModel* m, int param) { return m ? model_param_dim(&m->desc, param) : -1; }

int mjl_batch_set_model_params(mjlBatch* B, const float* const* values, const float* mask, void* stream) {
  if (!B || !values) return fail(MJL_ERR_ARG, "null argument");
  if (!B->d_model_env) return fail(MJL_ERR_ARG, "MJL_OPT_PER_ENV_MODEL not set");
  HIPCHK(hipSetDevice(B->device));
  return launch_model_params(B, values, mask, 0, stream);
}

int mjl_batch_get_model_params(mjlBatch* B, int param, float* dst, void* stream) {
  if (!B || !dst) return fail(MJL_ERR_ARG, "null argument");
  if (!B->d_model_env) return fail(MJL_ERR_ARG, "MJL_OPT_PER_ENV_MODEL not set");
  const int dim = model_param_dim(&B->model->desc, param);
  if (dim < 0) return fail(MJL_ERR_ARG, "unknown model parameter %d", param);
  if (dim == 0) return MJL_OK;
  HIPCHK(hipSetDevice(B->device));
  const long n = (long)B->nenv * dim;
  hipLaunchKernelGGL(model_params_get_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const ModelF*)B->d_model_env, param, B->nenv, dim, dst);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

}  // extern "C"

__global__ void masked_copy_kernel(float* dst, const float* src, const float* mask, int nenv, int dim) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long n = (long)nenv * dim;
  if (i >= n) return;
  int env = (int)(i / dim);
  if (!mask || mask[env] > 0.5f) dst[i] = src[i];
}

extern "C" int mjl_get(mjlBatch* B, int field, float* dst, void* stream) {
  if (!B || !dst || field < 0 || field >= MJL_NFIELD) return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  HIPCHK(hipMemcpyAsync(dst, B->field_ptr[field], sizeof(float) * (size_t)B->dim[field] * B->nenv,
                        hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MJL_OK;
}

extern "C" int mjl_set(mjlBatch* B, int field, const float* src, const float* mask, void* stream) {
  if (!B || !src || field < 0 || field >= MJL_NFIELD) return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  long n = (long)B->dim[field] * B->nenv;
  if (!mask) {
    HIPCHK(hipMemcpyAsync(B->field_ptr[field], src, sizeof(float) * n, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  } else {
    int threads = 256;
    long blocks = (n + threads - 1) / threads;
    hipLaunchKernelGGL(masked_copy_kernel, dim3((unsigned)blocks), dim3(threads), 0, (hipStream_t)stream,
                       B->field_ptr[field], src, mask, B->nenv, B->dim[field]);
    HIPCHK(hipGetLastError());
  }
  return MJL_OK;
}

// packed persistent state rows [qpos | qvel | qacc_warmstart | aux | time] (APG tape)
__global__ void pack_state_kernel(StateBuf S, int nenv, int nq, int nv, float* __restrict__ dst) {
  const int w = nq + 2 * nv + MJL_AUX_DIM + 1;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)nenv * w) return;
  const int e = (int)(t / w), k = (int)(t % w);
  float v;
  if (k < nq) v = S.qpos[(size_t)e * nq + k];
  else if (k < nq + nv) v = S.qvel[(size_t)e * nv + k - nq];
  else if (k < nq + 2 * nv) v = S.qacc_warmstart[(size_t)e * nv + k - nq - nv];
  else if (k < nq + 2 * nv + MJL_AUX_DIM) v = S.aux[(size_t)e * MJL_AUX_DIM + k - nq - 2 * nv];
  else v = S.time[e];
  dst[t] = v;
}
__global__ void unpack_state_kernel(StateBuf S, int nenv, int nq, int nv, const float* __restrict__ src,
                                    const float* __restrict__ ws_src) {
  const int w = nq + 2 * nv + MJL_AUX_DIM + 1;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long)nenv * w) return;
  const int e = (int)(t / w), k = (int)(t % w);
  const float v = src[t];
  if (k < nq) S.qpos[(size_t)e * nq + k] = v;
  else if (k < nq + nv) S.qvel[(size_t)e * nv + k - nq] = v;
  else if (k < nq + 2 * nv) S.qacc_warmstart[(size_t)e * nv + k - nq - nv] = ws_src ? ws_src[t] : v;
  else if (k < nq + 2 * nv + MJL_AUX_DIM) S.aux[(size_t)e * MJL_AUX_DIM + k - nq - 2 * nv] = v;
  else S.time[e] = v;
}

extern "C" int mjl_state_size(const mjlBatch* B) {
  if (!B) return -1;
  return B->model->desc.nq + 2 * B->model->desc.nv + MJL_AUX_DIM + 1;
}

extern "C" int mjl_get_state(mjlBatch* B, float* dst, void* stream) {
  if (!B || !dst) return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  const long n = (long)B->nenv * (nq + 2 * nv + MJL_AUX_DIM + 1);
  hipLaunchKernelGGL(pack_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B->s,
                     B->nenv, nq, nv, dst);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_set_state(mjlBatch* B, const float* src, const float* ws_src, void* stream) {
  if (!B || !src) return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  const long n = (long)B->nenv * (nq + 2 * nv + MJL_AUX_DIM + 1);
  hipLaunchKernelGGL(unpack_state_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B->s,
                     B->nenv, nq, nv, src, ws_src);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

static KParams make_params(mjlBatch* B) {
  KParams P;
  std::memset(&P, 0, sizeof(P));
  P.pool_slot = -1;
  P.m = B->d_model;
  P.env = B->d_env;
  P.s = B->s;
  P.nenv = B->nenv;
  P.store_derived = B->store_derived;
  P.force_global_rows = B->force_global_rows;
  P.scratch = B->d_scratch;
  P.scratch_stride = B->scratch_stride;
  P.gmax_efc = B->gmax_efc;
  P.gmax_con = B->gmax_con;
  P.ctr_base = B->ctr_base;
  P.keys = B->reset_keys;
  P.key_mode = B->key_mode;
  return P;
}

static void set_seed_counter(KParams& P, uint64_t seed, uint64_t counter) {
  P.seed_lo = (uint32_t)seed; P.seed_hi = (uint32_t)(seed >> 32);
  P.ctr_lo = (uint32_t)counter; P.ctr_hi = (uint32_t)(counter >> 32);
}

// env-step launches of at most one wave per SIMD (nenv <= 4 x CUs: C3's 1024-env rollout) take the
// one-wave instantiation (MJL_ONE_WAVE=0 disables it, for A/B runs). Measured (profiles/r4_onewave_ab.jsonl,
// interleaved): pooled env step at 1024 envs 81.4 -> 77.0 us, in-place 109.5 -> 106.4 us; the speed test
// at 1024 envs ran 2 % slower one-wave (55.6 -> 56.7 us), so it keeps the two-wave kernel.
static bool one_wave_launch(const mjlBatch* B) {
  static const bool on = [] { const char* e = std::getenv("MJL_ONE_WAVE"); return !(e && e[0] == '0'); }();
  return on && B->nenv <= B->simds;
}

// APPLIED: the launch honours the batch's attached applied forces (forward, step and env step; every
// other launch runs with zero applied force, whatever is attached). Nothing attached: the plain kernels.
// With MJL_OPT_PER_ENV_MODEL on, every launch but the speed test's takes the per-env instantiation: forward,
// step and env step the applied one too (null buffers when nothing is attached: the plain computation), so
// that pushes and randomisation combine without a third set of kernels; the reset the plain one. (No one-wave
// variant, as for the applied kernels.)
template <int MODE, bool APPLIED = false> static int launch(mjlBatch* B, const KParams& P0, void* stream) {
  HIPCHK(hipSetDevice(B->device));
  dim3 grid(B->nenv), block(64);
  constexpr bool kOneWave = MODE == MODE_ENV_STEP;
  if constexpr (MODE != MODE_SPEEDTEST) {
    if (B->d_model_env) {
      KParams P = P0;
      P.m_env = B->d_model_env;
      if constexpr (APPLIED) { P.qfrc_applied = B->qfrc_applied; P.xfrc_applied = B->xfrc_applied; }
      constexpr int kMode = MODE | MODE_PER_ENV | (APPLIED ? MODE_APPLIED : 0);
      if (B->model->nvc == 0)
        hipLaunchKernelGGL((step_kernel<DHum, kMode>), grid, block, 0, (hipStream_t)stream, P);
      else
        hipLaunchKernelGGL((step_kernel<DGen, kMode>), grid, block, 0, (hipStream_t)stream, P);
      HIPCHK(hipGetLastError());
      return MJL_OK;
    }
  }
  if constexpr (APPLIED) {
    if (B->qfrc_applied || B->xfrc_applied) {
      KParams P = P0;
      P.qfrc_applied = B->qfrc_applied; P.xfrc_applied = B->xfrc_applied;
      // (no one-wave instantiation: a second caller of the one-wave env_reset / global_rows_path changed the
      // code the compiler makes for them and for the plain one-wave env step)
      constexpr int kMode = MODE | MODE_APPLIED;
      if (B->model->nvc == 0)
        hipLaunchKernelGGL((step_kernel<DHum, kMode>), grid, block, 0, (hipStream_t)stream, P);
      else
        hipLaunchKernelGGL((step_kernel<DGen, kMode>), grid, block, 0, (hipStream_t)stream, P);
      HIPCHK(hipGetLastError());
      return MJL_OK;
    }
  }
  const KParams& P = P0;
  if (B->model->nvc == 0 && kOneWave && one_wave_launch(B))
    hipLaunchKernelGGL((step_kernel<DHum, MODE, kOneWave ? 1 : MJL_MINWAVES>), grid, block, 0, (hipStream_t)stream, P);
  else if (B->model->nvc == 0)
    hipLaunchKernelGGL((step_kernel<DHum, MODE>), grid, block, 0, (hipStream_t)stream, P);
  else
    hipLaunchKernelGGL((step_kernel<DGen, MODE>), grid, block, 0, (hipStream_t)stream, P);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" {

int mjl_forward(mjlBatch* B, const float* mask, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  KParams P = make_params(B);
  P.mask = mask;
  return launch<MODE_FORWARD, true>(B, P, stream);
}

// Two launches: the forward pass with this call's rows in the global slab (the batch's
// MJL_OPT_FORCE_GLOBAL_ROWS option is not touched), then the readout of that slab (contact_kernels.hip).
int mjl_forward_contacts(mjlBatch* B, const float* mask, int max_con, int32_t* ncon, int32_t* geom, int32_t* dim,
                         int32_t* efc_adr, float* dist, float* pos, float* frame, float* force, float* body_force,
                         void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!ncon) return fail(MJL_ERR_ARG, "ncon is required");
  if (max_con < 1) return fail(MJL_ERR_ARG, "max_con must be >= 1");
  KParams P = make_params(B);
  P.mask = mask;
  P.force_global_rows = 1;
  if (int rc = launch<MODE_FORWARD, true>(B, P, stream)) return rc;
  ContactOut O;
  O.ncon = ncon; O.geom = geom; O.dim = dim; O.efc_adr = efc_adr;
  O.dist = dist; O.pos = pos; O.frame = frame; O.force = force; O.body_force = body_force;
  O.max_con = max_con;
  dim3 grid(B->nenv), block(64);
  // The shared block also with MJL_OPT_PER_ENV_MODEL on: of the model, contacts_kernel reads prec[].g1 / g2 /
  // includemargin and nbody, none of them a per-env field, and takes mu from the contact record the (per-env)
  // forward pass wrote. A read of a MJL_MP_* field added there needs the env's block (d_model_env + env).
  if (B->model->nvc == 0)
    hipLaunchKernelGGL(contacts_kernel<DHum>, grid, block, 0, (hipStream_t)stream, (const ModelF*)B->d_model,
                       (const float*)B->s.stats, mask, B->d_scratch, B->scratch_stride, B->gmax_efc, B->gmax_con,
                       B->nenv, O);
  else
    hipLaunchKernelGGL(contacts_kernel<DGen>, grid, block, 0, (hipStream_t)stream, (const ModelF*)B->d_model,
                       (const float*)B->s.stats, mask, B->d_scratch, B->scratch_stride, B->gmax_efc, B->gmax_con,
                       B->nenv, O);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// With the acc stage two launches, as mjl_forward_contacts: the forward pass with this call's rows in the global
// slab, then the readout (sensor_kernels.hip), which reads the derived store and the limit rows. Without it
// the readout alone, from qpos / qvel and the model.
int mjl_sensors(mjlBatch* B, const float* mask, int stages, float* out, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!out) return fail(MJL_ERR_ARG, "out is required");
  const int all = MJL_SENS_STAGE_POS | MJL_SENS_STAGE_VEL | MJL_SENS_STAGE_ACC;
  if (stages == 0 || (stages & ~all)) return fail(MJL_ERR_ARG, "stages = %d: a nonzero mask of MJL_SENS_STAGE_*", stages);
  if (!B->d_sensors) return MJL_OK;  // no readout sensors
  if (stages & MJL_SENS_STAGE_ACC) {
    KParams P = make_params(B);
    P.mask = mask;
    P.force_global_rows = 1;
    if (int rc = launch<MODE_FORWARD, true>(B, P, stream)) return rc;
  } else {
    HIPCHK(hipSetDevice(B->device));
  }
  SensorArgs A;
  A.m = B->d_model; A.m_env = B->d_model_env; A.tab = B->d_sensors; A.s = B->s; A.mask = mask;
  A.scratch = B->d_scratch; A.scratch_stride = B->scratch_stride; A.gmax_efc = B->gmax_efc; A.gmax_con = B->gmax_con;
  A.LD = B->model->nvc == 0 ? DHum::LD : DGen::LD;
  A.nenv = B->nenv; A.stages = stages; A.out = out;
  hipLaunchKernelGGL(sensors_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// With a cfrc output two launches, as mjl_sensors with its acc stage: the forward pass with this call's rows in
// the global slab, then the readout (body_kernels.hip), which reads qacc, the contact count and the slab's
// contacts. Without one the readout alone, from qpos / qvel and the model.
int mjl_body_data(mjlBatch* B, const float* mask, float* xipos, float* ximat, float* subtree_com, float* cinert,
                  float* cvel, float* subtree_linvel, float* subtree_angmom, float* cfrc_ext, float* cfrc_int,
                  void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!xipos && !ximat && !subtree_com && !cinert && !cvel && !subtree_linvel && !subtree_angmom && !cfrc_ext &&
      !cfrc_int)
    return fail(MJL_ERR_ARG, "mjl_body_data: every output is NULL");
  if (cfrc_ext || cfrc_int) {
    KParams P = make_params(B);
    P.mask = mask;
    P.force_global_rows = 1;
    if (int rc = launch<MODE_FORWARD, true>(B, P, stream)) return rc;
  } else {
    HIPCHK(hipSetDevice(B->device));
  }
  BodyArgs A;
  A.m = B->d_model; A.m_env = B->d_model_env; A.tab = B->d_bodytab; A.s = B->s; A.mask = mask;
  A.xfrc = B->xfrc_applied;
  A.scratch = B->d_scratch; A.scratch_stride = B->scratch_stride; A.gmax_efc = B->gmax_efc; A.gmax_con = B->gmax_con;
  A.nenv = B->nenv;
  A.xipos = xipos; A.ximat = ximat; A.subtree_com = subtree_com; A.cinert = cinert; A.cvel = cvel;
  A.subtree_linvel = subtree_linvel; A.subtree_angmom = subtree_angmom; A.cfrc_ext = cfrc_ext; A.cfrc_int = cfrc_int;
  if (B->model->nvc == 0)
    hipLaunchKernelGGL(body_data_kernel<DHum>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(body_data_kernel<DGen>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// One launch each (dyn_kernels.hip): forward kinematics of the current qpos inside the kernel, nothing of the
// batch written.
int mjl_jac(mjlBatch* B, const float* mask, int npoint, const int32_t* body, int frame, const float* pnt, float* jacp,
            float* jacr, float* xpnt, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!body) return fail(MJL_ERR_ARG, "mjl_jac: body is required");
  if (!jacp && !jacr) return fail(MJL_ERR_ARG, "mjl_jac: jacp and jacr are both NULL");
  if (npoint < 1 || npoint > 256) return fail(MJL_ERR_ARG, "mjl_jac: npoint = %d outside 1..256", npoint);
  if (frame != MJL_JAC_WORLD && frame != MJL_JAC_LOCAL)
    return fail(MJL_ERR_ARG, "mjl_jac: frame = %d: MJL_JAC_WORLD or MJL_JAC_LOCAL", frame);
  if (frame == MJL_JAC_WORLD && !pnt) return fail(MJL_ERR_ARG, "mjl_jac: pnt is required with MJL_JAC_WORLD");
  HIPCHK(hipSetDevice(B->device));
  JacArgs A;
  A.m = B->d_model; A.tab = B->d_dyntab; A.qpos = B->s.qpos; A.mask = mask;
  A.nenv = B->nenv; A.npoint = npoint; A.frame = frame; A.body = body; A.pnt = pnt;
  A.jacp = jacp; A.jacr = jacr; A.xpnt = xpnt;
  hipLaunchKernelGGL(jac_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_mass_matrix(mjlBatch* B, const float* mask, float* full_m, int nvec, const float* vec, float* mul_m,
                    float* solve_m, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!full_m && !mul_m && !solve_m) return fail(MJL_ERR_ARG, "mjl_mass_matrix: every output is NULL");
  if (nvec < 0 || nvec > 64) return fail(MJL_ERR_ARG, "mjl_mass_matrix: nvec = %d outside 0..64", nvec);
  if (mul_m || solve_m) {
    if (!vec) return fail(MJL_ERR_ARG, "mjl_mass_matrix: vec is required with mul_m or solve_m");
    if (nvec < 1) return fail(MJL_ERR_ARG, "mjl_mass_matrix: nvec = 0 with mul_m or solve_m");
  }
  HIPCHK(hipSetDevice(B->device));
  MassArgs A;
  A.m = B->d_model; A.m_env = B->d_model_env; A.qpos = B->s.qpos; A.mask = mask;
  A.nenv = B->nenv; A.nvec = nvec; A.vec = vec; A.full_m = full_m; A.mul_m = mul_m; A.solve_m = solve_m;
  hipLaunchKernelGGL(mass_matrix_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// One launch each (taskspace_kernels.hip): kinematics and rates of the current qpos / qvel inside the kernel,
// nothing of the batch written.
int mjl_jac_dot(mjlBatch* B, const float* mask, int npoint, const int32_t* body, int frame, const float* pnt,
                float* jacp_dot, float* jacr_dot, float* jdotv, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!body) return fail(MJL_ERR_ARG, "mjl_jac_dot: body is required");
  if (!jacp_dot && !jacr_dot && !jdotv) return fail(MJL_ERR_ARG, "mjl_jac_dot: every output is NULL");
  if (npoint < 1 || npoint > 256) return fail(MJL_ERR_ARG, "mjl_jac_dot: npoint = %d outside 1..256", npoint);
  if (frame != MJL_JAC_WORLD && frame != MJL_JAC_LOCAL)
    return fail(MJL_ERR_ARG, "mjl_jac_dot: frame = %d: MJL_JAC_WORLD or MJL_JAC_LOCAL", frame);
  if (frame == MJL_JAC_WORLD && !pnt) return fail(MJL_ERR_ARG, "mjl_jac_dot: pnt is required with MJL_JAC_WORLD");
  HIPCHK(hipSetDevice(B->device));
  JacDotArgs A;
  A.m = B->d_model; A.tab = B->d_dyntab; A.qpos = B->s.qpos; A.qvel = B->s.qvel; A.mask = mask;
  A.nenv = B->nenv; A.npoint = npoint; A.frame = frame; A.body = body; A.pnt = pnt;
  A.jacp_dot = jacp_dot; A.jacr_dot = jacr_dot; A.jdotv = jdotv;
  hipLaunchKernelGGL(jac_dot_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_centroidal(mjlBatch* B, const float* mask, int nsub, const int32_t* body, float* jac_com, float* angmom_mat,
                   float* bias, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!body) return fail(MJL_ERR_ARG, "mjl_centroidal: body is required");
  if (!jac_com && !angmom_mat && !bias) return fail(MJL_ERR_ARG, "mjl_centroidal: every output is NULL");
  if (nsub < 1 || nsub > 32) return fail(MJL_ERR_ARG, "mjl_centroidal: nsub = %d outside 1..32", nsub);
  HIPCHK(hipSetDevice(B->device));
  CentArgs A;
  A.m = B->d_model; A.m_env = B->d_model_env; A.tab = B->d_dyntab; A.qpos = B->s.qpos; A.qvel = B->s.qvel;
  A.mask = mask; A.nenv = B->nenv; A.nsub = nsub; A.body = body;
  A.jac_com = jac_com; A.angmom_mat = angmom_mat; A.bias = bias;
  hipLaunchKernelGGL(centroidal_kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// One launch each (ik_kernels.hip): every iteration of every env's solve on chip, nothing of the batch written.
// The checks of the scalars mjl_ik and mjl_ik_wb share (fn: the entry's name in the message).
static int ik_check_scalars(const char* fn, int iterations, float damping, float posture, float max_step, float tol,
                            int flags) {
  if (iterations < 0 || iterations > 1024) return fail(MJL_ERR_ARG, "%s: iterations = %d outside 0..1024", fn, iterations);
  if (!(damping > 0.f) || !std::isfinite(damping)) return fail(MJL_ERR_ARG, "%s: damping = %g: a finite value > 0", fn, damping);
  if (!(posture >= 0.f) || !std::isfinite(posture)) return fail(MJL_ERR_ARG, "%s: posture = %g: a finite value >= 0", fn, posture);
  if (!(max_step >= 0.f) || !std::isfinite(max_step)) return fail(MJL_ERR_ARG, "%s: max_step = %g: a finite value >= 0", fn, max_step);
  if (!(tol >= 0.f) || !std::isfinite(tol)) return fail(MJL_ERR_ARG, "%s: tol = %g: a finite value >= 0", fn, tol);
  if (flags & ~MJL_IK_LIMITS) return fail(MJL_ERR_ARG, "%s: flags = %d: 0 or MJL_IK_LIMITS", fn, flags);
  return MJL_OK;
}

static void ik_fill(IkArgs& A, mjlBatch* B, const float* mask, int ntask, const int32_t* body, const float* offset,
                    const float* target_pos, const float* target_quat, const float* weight, const float* qpos_start,
                    const float* qpos_ref, int32_t dofmask, int iterations, float damping, float posture,
                    float max_step, float tol, int flags, float* qpos_out, float* err, int32_t* niter) {
  A.m = B->d_model; A.tab = B->d_dyntab; A.qstart = qpos_start ? qpos_start : B->s.qpos; A.qref = qpos_ref;
  A.mask = mask; A.nenv = B->nenv; A.ntask = ntask; A.body = body; A.offset = offset; A.tpos = target_pos;
  A.tquat = target_quat; A.weight = weight; A.dofmask = (uint32_t)dofmask; A.iterations = iterations;
  A.limits = (flags & MJL_IK_LIMITS) != 0; A.damping = damping; A.posture = posture; A.max_step = max_step; A.tol = tol;
  A.qout = qpos_out; A.err = err; A.niter = niter;
}

int mjl_ik(mjlBatch* B, const float* mask, int ntask, const int32_t* body, const float* offset, const float* target_pos,
           const float* target_quat, const float* weight, const float* qpos_start, const float* qpos_ref,
           int32_t dofmask, int iterations, float damping, float posture, float max_step, float tol, int flags,
           float* qpos_out, float* err, int32_t* niter, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!body) return fail(MJL_ERR_ARG, "mjl_ik: body is required");
  if (!qpos_out) return fail(MJL_ERR_ARG, "mjl_ik: qpos_out is required");
  if (ntask < 1 || ntask > kIkMaxTask) return fail(MJL_ERR_ARG, "mjl_ik: ntask = %d outside 1..%d", ntask, kIkMaxTask);
  if (!target_pos && !target_quat) return fail(MJL_ERR_ARG, "mjl_ik: target_pos and target_quat are both NULL");
  if (int rc = ik_check_scalars("mjl_ik", iterations, damping, posture, max_step, tol, flags)) return rc;
  HIPCHK(hipSetDevice(B->device));
  IkArgs A;
  ik_fill(A, B, mask, ntask, body, offset, target_pos, target_quat, weight, qpos_start, qpos_ref, dofmask, iterations,
          damping, posture, max_step, tol, flags, qpos_out, err, niter);
  hipLaunchKernelGGL(ik_kernel<false>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_ik_wb(mjlBatch* B, const float* mask, int ntask, const int32_t* body, const float* offset,
              const float* target_pos, const float* target_quat, const float* weight, const float* qpos_start,
              const float* qpos_ref, int32_t dofmask, int iterations, float damping, float posture, float max_step,
              float tol, int flags, float* qpos_out, float* err, int32_t* niter, int com_body, const float* com_target,
              const float* com_weight, int npair, const int32_t* geom1, const int32_t* geom2, const float* clear_min,
              const float* clear_weight, float* com_err, float* clearance, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!qpos_out) return fail(MJL_ERR_ARG, "mjl_ik_wb: qpos_out is required");
  if (ntask < 0 || ntask > kIkMaxTask) return fail(MJL_ERR_ARG, "mjl_ik_wb: ntask = %d outside 0..%d", ntask, kIkMaxTask);
  if (ntask > 0 && !body) return fail(MJL_ERR_ARG, "mjl_ik_wb: body is required with ntask > 0");
  if (ntask > 0 && !target_pos && !target_quat)
    return fail(MJL_ERR_ARG, "mjl_ik_wb: target_pos and target_quat are both NULL with ntask > 0");
  if (int rc = ik_check_scalars("mjl_ik_wb", iterations, damping, posture, max_step, tol, flags)) return rc;
  const mjlModelDesc& d = B->model->desc;
  if (com_body < -1 || com_body >= d.nbody)
    return fail(MJL_ERR_ARG, "mjl_ik_wb: com_body = %d outside -1..%d", com_body, d.nbody - 1);
  if (com_body >= 0 && !com_target) return fail(MJL_ERR_ARG, "mjl_ik_wb: com_target is required with com_body >= 0");
  if (npair < 0 || npair > kIkMaxPair) return fail(MJL_ERR_ARG, "mjl_ik_wb: npair = %d outside 0..%d", npair, kIkMaxPair);
  if (ntask == 0 && com_body < 0 && npair == 0) return fail(MJL_ERR_ARG, "mjl_ik_wb: no task of any kind");
  if (npair > 0 && (!geom1 || !geom2 || !clear_min))
    return fail(MJL_ERR_ARG, "mjl_ik_wb: geom1, geom2 and clear_min are required with npair > 0");
  IkWbArgs A;
  for (int i = 0; i < 3; i++) {
    const float w = com_weight ? com_weight[i] : 1.f;
    if (com_body >= 0 && (!(w >= 0.f) || !std::isfinite(w)))
      return fail(MJL_ERR_ARG, "mjl_ik_wb: com_weight[%d] = %g: a finite value >= 0", i, w);
    A.com_weight[i] = w;
  }
  for (int p = 0; p < kIkMaxPair; p++) {
    A.geom1[p] = A.geom2[p] = 0;
    A.clear_min[p] = A.clear_weight[p] = 0.f;
  }
  if (npair > 0)
    for (int g = 0; g < d.ngeom; g++)
      if (d.geom_type[g] != MJL_GEOM_PLANE && d.geom_type[g] != MJL_GEOM_SPHERE && d.geom_type[g] != MJL_GEOM_CAPSULE)
        return fail(MJL_ERR_UNSUPPORTED, "mjl_ik_wb: geom %d has type %d (plane, sphere and capsule have closed forms)",
                    g, d.geom_type[g]);
  for (int p = 0; p < npair; p++) {
    const int g1 = geom1[p], g2 = geom2[p];
    const int ng = d.ngeom < MJL_MAXGEOM ? d.ngeom : MJL_MAXGEOM;
    if (g1 < 0 || g1 >= ng || g2 < 0 || g2 >= ng)
      return fail(MJL_ERR_ARG, "mjl_ik_wb: pair %d: geoms %d, %d outside 0..%d", p, g1, g2, ng - 1);
    if (g1 == g2) return fail(MJL_ERR_ARG, "mjl_ik_wb: pair %d: geom %d is paired with itself", p, g1);
    if (d.geom_type[g1] == MJL_GEOM_PLANE && d.geom_type[g2] == MJL_GEOM_PLANE)
      return fail(MJL_ERR_ARG, "mjl_ik_wb: pair %d: geoms %d and %d are both planes", p, g1, g2);
    const float w = clear_weight ? clear_weight[p] : 1.f;
    if (!(w >= 0.f) || !std::isfinite(w)) return fail(MJL_ERR_ARG, "mjl_ik_wb: clear_weight[%d] = %g: a finite value >= 0", p, w);
    if (!(clear_min[p] >= 0.f) || !std::isfinite(clear_min[p]))
      return fail(MJL_ERR_ARG, "mjl_ik_wb: clear_min[%d] = %g: a finite value >= 0", p, clear_min[p]);
    A.geom1[p] = (uint8_t)g1; A.geom2[p] = (uint8_t)g2; A.clear_min[p] = clear_min[p]; A.clear_weight[p] = w;
  }
  HIPCHK(hipSetDevice(B->device));
  ik_fill(A, B, mask, ntask, body, offset, target_pos, target_quat, weight, qpos_start, qpos_ref, dofmask, iterations,
          damping, posture, max_step, tol, flags, qpos_out, err, niter);
  A.m_env = B->d_model_env; A.com_target = com_target; A.com_body = com_body; A.npair = npair;
  A.com_err = com_err; A.clearance = clearance;
  hipLaunchKernelGGL(ik_kernel<true>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// One launch (inverse_kernels.hip): the forward pass's smooth phases and rows, no solver, nothing of the batch written.
int mjl_inverse(mjlBatch* B, const float* mask, const float* qacc, int flags, float* qfrc_inverse,
                float* qfrc_constraint, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!qfrc_inverse) return fail(MJL_ERR_ARG, "mjl_inverse: qfrc_inverse is required");
  if (flags & ~MJL_INV_DISCRETE) return fail(MJL_ERR_ARG, "mjl_inverse: flags = %d: 0 or MJL_INV_DISCRETE", flags);
  HIPCHK(hipSetDevice(B->device));
  InvArgs A;
  A.m = B->d_model; A.m_env = B->d_model_env; A.qpos = B->s.qpos; A.qvel = B->s.qvel;
  A.qacc = qacc ? qacc : B->s.qacc; A.mask = mask;
  A.qfrc_inverse = qfrc_inverse; A.qfrc_constraint = qfrc_constraint;
  A.scratch = B->d_scratch; A.scratch_stride = B->scratch_stride; A.gmax_efc = B->gmax_efc; A.gmax_con = B->gmax_con;
  A.nenv = B->nenv; A.flags = flags; A.force_global_rows = B->force_global_rows;
  if (B->model->nvc == 0)
    hipLaunchKernelGGL(inverse_kernel<DHum>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(inverse_kernel<DGen>, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// Rays per wavefront of rays_kernel (ray_kernels.hip) unless MJL_OPT_RAY_CHUNK says otherwise: every chunk's
// wavefront repeats the env's kinematics. DESIGN.md "Rays" has the measurement behind the value.
constexpr int kRayChunk = 64;

// the checks mjl_ray and mjl_ray_scan share, then the launch
static int launch_rays(mjlBatch* B, RayArgs& A, void* stream) {
  const mjlModelDesc& d = B->model->desc;
  if (A.nray < 1 || A.nray > 65535) return fail(MJL_ERR_ARG, "nray = %d outside 1..65535", A.nray);
  if (A.flags & ~MJL_RAY_STATIC) return fail(MJL_ERR_ARG, "flags = %d: unknown bits (MJL_RAY_STATIC)", A.flags);
  if (A.bodyexclude < -1 || A.bodyexclude >= d.nbody)
    return fail(MJL_ERR_ARG, "bodyexclude = %d outside -1..%d", A.bodyexclude, d.nbody - 1);
  for (int g = 0; g < d.ngeom; g++)
    if (d.geom_type[g] != MJL_GEOM_PLANE && d.geom_type[g] != MJL_GEOM_SPHERE && d.geom_type[g] != MJL_GEOM_CAPSULE)
      return fail(MJL_ERR_UNSUPPORTED, "rays: geom %d has type %d (plane, sphere and capsule are tested)", g,
                  d.geom_type[g]);
  A.m = B->d_model; A.qpos = B->s.qpos; A.nenv = B->nenv;
  A.chunk = B->ray_chunk > 0 ? B->ray_chunk : kRayChunk;
  A.nchunk = (A.nray + A.chunk - 1) / A.chunk;
  const long long blocks = (long long)B->nenv * A.nchunk;
  if (blocks > 0x7fffffffLL) return fail(MJL_ERR_ARG, "rays: %d envs x %d ray chunks exceed one launch", B->nenv, A.nchunk);
  HIPCHK(hipSetDevice(B->device));
  hipLaunchKernelGGL(rays_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_ray(mjlBatch* B, const float* mask, int nray, const float* pnt, const float* vec, int flags, int bodyexclude,
            float cutoff, float* dist, int32_t* geomid, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!dist) return fail(MJL_ERR_ARG, "dist is required");
  if (!pnt) return fail(MJL_ERR_ARG, "pnt is required");
  if (!vec) return fail(MJL_ERR_ARG, "vec is required");
  RayArgs A = {};
  A.mask = mask; A.pnt = pnt; A.vec = vec; A.nray = nray; A.scan = 0;
  A.flags = flags; A.bodyexclude = bodyexclude; A.cutoff = cutoff;
  A.dist = dist; A.geomid = geomid; A.hitpos = nullptr;
  return launch_rays(B, A, stream);
}

int mjl_ray_scan(mjlBatch* B, const float* mask, int objtype, int objid, int align, int nray, const float* lpnt,
                 const float* lvec, int flags, int bodyexclude, float cutoff, float* dist, int32_t* geomid,
                 float* hitpos, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!dist) return fail(MJL_ERR_ARG, "dist is required");
  if (!lpnt) return fail(MJL_ERR_ARG, "lpnt is required");
  if (!lvec) return fail(MJL_ERR_ARG, "lvec is required");
  const mjlModelDesc& d = B->model->desc;
  if (objtype != MJL_OBJ_XBODY && objtype != MJL_OBJ_SITE)
    return fail(MJL_ERR_ARG, "objtype = %d: MJL_OBJ_XBODY or MJL_OBJ_SITE", objtype);
  const int nobj = objtype == MJL_OBJ_XBODY ? d.nbody : d.nsite;
  if (objid < 0 || objid >= nobj) return fail(MJL_ERR_ARG, "objid = %d outside 0..%d", objid, nobj - 1);
  if (align != MJL_SCAN_POSE && align != MJL_SCAN_YAW) return fail(MJL_ERR_ARG, "align = %d: MJL_SCAN_POSE or MJL_SCAN_YAW", align);
  RayArgs A = {};
  A.mask = mask; A.pnt = lpnt; A.vec = lvec; A.nray = nray; A.scan = 1;
  A.objtype = objtype; A.objid = objid; A.align = align;
  A.flags = flags; A.bodyexclude = bodyexclude; A.cutoff = cutoff;
  A.dist = dist; A.geomid = geomid; A.hitpos = hitpos;
  return launch_rays(B, A, stream);
}

// Pairs per wavefront of geom_distance_kernel (distance_kernels.hip) unless MJL_OPT_DISTANCE_CHUNK says otherwise:
// every chunk's wavefront repeats the env's kinematics. DESIGN.md "Geom distance" has the measurement behind the value.
constexpr int kDistChunk = 64;

// One launch (distance_kernels.hip): forward kinematics of the current qpos inside the kernel, nothing of the
// batch written.
int mjl_geom_distance(mjlBatch* B, const float* mask, int npair, const int32_t* geom1, const int32_t* geom2,
                      float distmax, float* dist, float* fromto, float* normal, float* jac, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!dist) return fail(MJL_ERR_ARG, "mjl_geom_distance: dist is required");
  if (!geom1 || !geom2) return fail(MJL_ERR_ARG, "mjl_geom_distance: geom1 and geom2 are required");
  if (npair < 1 || npair > 65535) return fail(MJL_ERR_ARG, "mjl_geom_distance: npair = %d outside 1..65535", npair);
  if (!(distmax > 0.f)) return fail(MJL_ERR_ARG, "mjl_geom_distance: distmax = %g: a value > 0 (+inf: no cap)", distmax);
  const mjlModelDesc& d = B->model->desc;
  for (int g = 0; g < d.ngeom; g++)
    if (d.geom_type[g] != MJL_GEOM_PLANE && d.geom_type[g] != MJL_GEOM_SPHERE && d.geom_type[g] != MJL_GEOM_CAPSULE)
      return fail(MJL_ERR_UNSUPPORTED, "mjl_geom_distance: geom %d has type %d (plane, sphere and capsule have closed forms)",
                  g, d.geom_type[g]);
  DistArgs A;
  A.m = B->d_model; A.tab = B->d_dyntab; A.qpos = B->s.qpos; A.mask = mask;
  A.nenv = B->nenv; A.npair = npair;
  A.chunk = B->dist_chunk > 0 ? B->dist_chunk : kDistChunk;
  A.nchunk = (npair + A.chunk - 1) / A.chunk;
  A.geom1 = geom1; A.geom2 = geom2; A.distmax = distmax;
  A.dist = dist; A.fromto = fromto; A.normal = normal; A.jac = jac;
  const long long blocks = (long long)B->nenv * A.nchunk;
  if (blocks > 0x7fffffffLL)
    return fail(MJL_ERR_ARG, "mjl_geom_distance: %d envs x %d pair chunks exceed one launch", B->nenv, A.nchunk);
  HIPCHK(hipSetDevice(B->device));
  hipLaunchKernelGGL(geom_distance_kernel, dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_step(mjlBatch* B, const float* ctrl, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  KParams P = make_params(B);
  P.in_ctrl = ctrl;
  return launch<MODE_STEP, true>(B, P, stream);
}

int mjl_step_n(mjlBatch* B, const float* ctrl, int nstep, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (nstep < 1 || nstep > MJL_MAXSUBSTEP) return fail(MJL_ERR_ARG, "nstep = %d outside 1..%d", nstep, MJL_MAXSUBSTEP);
  // nstep single-step launches (see substep_kernels.hip); the first stores ctrl, the others run the stored one
  if (int rc = mjl_step(B, ctrl, stream)) return rc;
  for (int s = 1; s < nstep; s++)
    if (int rc = mjl_step(B, nullptr, stream)) return rc;
  return MJL_OK;
}

int mjl_speedtest_step(mjlBatch* B, const float* vel, float* out, void* stream) {
  if (!B || !vel || !out) return fail(MJL_ERR_ARG, "bad argument");
  KParams P = make_params(B);
  P.vel = vel;
  P.out_speed = out;
  P.store_derived = 0;
  return launch<MODE_SPEEDTEST>(B, P, stream);
}

int mjl_env_config(mjlBatch* B, const mjlEnvConfig* cfg) {
  if (!B || !cfg) return fail(MJL_ERR_ARG, "bad argument");
  const mjlModelDesc& d = B->model->desc;
  if (cfg->obs_dim <= 0 || cfg->obs_dim > 64) return fail(MJL_ERR_ARG, "obs_dim must be in 1..64");
  if (cfg->obs_dim != 1 + 3 + (d.nq - 7) + d.nv + 2) return fail(MJL_ERR_ARG, "obs_dim does not match the model");
  if (cfg->pelvis_body_id <= 0 || cfg->pelvis_body_id >= d.nbody || cfg->head_body_id <= 0 ||
      cfg->head_body_id >= d.nbody)
    return fail(MJL_ERR_ARG, "pelvis/head body id out of range");
  if (cfg->touch_sensor_right_id < 0 || cfg->touch_sensor_right_id >= d.nsensordata ||
      cfg->touch_sensor_left_id < 0 || cfg->touch_sensor_left_id >= d.nsensordata)
    return fail(MJL_ERR_ARG, "touch sensor id out of range");
  if (d.nbody < 2 || d.jnt_type[0] != MJL_JNT_FREE) return fail(MJL_ERR_UNSUPPORTED, "env needs a free-floating root");
  // the flip tables must be permutations: the action VJP writes each source's cotangent once
  // (adjoint.hip, o_ctrl[act_perm[lane]]), which covers every entry only for a bijection
  unsigned long long seen = 0;
  for (int i = 0; i < d.nu; i++) {
    if (cfg->act_perm[i] < 0 || cfg->act_perm[i] >= d.nu) return fail(MJL_ERR_ARG, "act_perm out of range");
    seen |= 1ull << cfg->act_perm[i];
  }
  if (seen != (d.nu == 64 ? ~0ull : (1ull << d.nu) - 1)) return fail(MJL_ERR_ARG, "act_perm is not a permutation");
  seen = 0;
  for (int i = 0; i < cfg->obs_dim; i++) {
    if (cfg->obs_perm[i] < 0 || cfg->obs_perm[i] >= cfg->obs_dim) return fail(MJL_ERR_ARG, "obs_perm out of range");
    seen |= 1ull << cfg->obs_perm[i];
  }
  if (seen != (cfg->obs_dim == 64 ? ~0ull : (1ull << cfg->obs_dim) - 1))
    return fail(MJL_ERR_ARG, "obs_perm is not a permutation");
  HIPCHK(hipSetDevice(B->device));
  HIPCHK(hipMemcpy(B->d_env, cfg, sizeof(mjlEnvConfig), hipMemcpyHostToDevice));
  if (B->d_pool_ctl) HIPCHK(hipMemset(B->d_pool_ctl, 0, (size_t)B->nenv * 2 * sizeof(int)));  // drawn under the old config
  B->has_env = 1;
  B->obs_dim = cfg->obs_dim;
  return MJL_OK;
}

int mjl_env_step(mjlBatch* B, const float* act, float* obs, float* rew, float* term, float* trunc, int auto_reset,
                 uint64_t seed, uint64_t counter, void* stream) {
  if (!B || !act || !obs || !rew || !term || !trunc) return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  KParams P = make_params(B);
  P.in_ctrl = act; P.obs = obs; P.rew = rew; P.term = term; P.trunc = trunc;
  P.auto_reset = auto_reset;
  set_seed_counter(P, seed, counter);
  if (B->d_pool_ctl && auto_reset) { P.rs = B->rs; P.rs_obs = B->rs_obs; P.pool_ctl = B->d_pool_ctl; }
  return launch<MODE_ENV_STEP, true>(B, P, stream);
}

int mjl_env_step_n(mjlBatch* B, const float* act, int nstep, float* obs, float* rew, float* term, float* trunc,
                   int auto_reset, uint64_t seed, uint64_t counter, void* stream) {
  if (!B || !act || !obs || !rew || !term || !trunc) return fail(MJL_ERR_ARG, "bad argument");
  if (nstep < 1 || nstep > MJL_MAXSUBSTEP) return fail(MJL_ERR_ARG, "nstep = %d outside 1..%d", nstep, MJL_MAXSUBSTEP);
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  if (nstep > 1) {  // the flipped and clipped action into the batch's ctrl, nstep - 1 plain steps on it
    HIPCHK(hipSetDevice(B->device));
    const int nu = B->model->desc.nu, n = B->nenv * nu;
    if (n > 0) {
      hipLaunchKernelGGL(env_ctrl_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B->d_env,
                         act, B->s.aux, B->s.ctrl, B->nenv, nu);
      HIPCHK(hipGetLastError());
    }
    for (int s = 1; s < nstep; s++)
      if (int rc = mjl_step(B, nullptr, stream)) return rc;
  }
  return mjl_env_step(B, act, obs, rew, term, trunc, auto_reset, seed, counter, stream);
}

int mjl_env_fill_reset_pool(mjlBatch* B, const int* dev_n, uint64_t seed, uint64_t counter, void* stream) {
  if (!B || !dev_n) return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  if (!B->d_pool_ctl) return fail(MJL_ERR_ARG, "MJL_OPT_RESET_POOL not set");
  if (B->reset_keys) return fail(MJL_ERR_ARG, "resets drawn from jax.random keys are not pooled");
  for (int j = 0; j < B->pool_slots; j++) {  // one launch per slot: each uses the batch's per-env scratch
    KParams P = make_params(B);
    const size_t rows = (size_t)j * B->nenv;
    P.s = B->rs;
    for (int f = 0; f < MJL_NFIELD; f++) P.s.*kStateField[f] += rows * B->dim[f];
    P.obs = B->rs_obs + rows * B->obs_dim;
    P.pool_ctl = B->d_pool_ctl; P.pool_n = dev_n; P.pool_slot = j; P.pool_slots = B->pool_slots;
    P.store_derived = 1;  // the consuming step may store derived fields
    // a counter domain of its own, the slot in bits 48..55: slot j + T of one rollout and slot j of the
    // next (counter + T) stay distinct for any rollout length T
    const uint64_t c = (counter + ((uint64_t)j << 48)) ^ (1ull << 63);
    set_seed_counter(P, seed, c);
    int rc = launch<MODE_ENV_RESET>(B, P, stream);
    if (rc != MJL_OK) return rc;
  }
  return MJL_OK;
}

int mjl_batch_set_counter_base(mjlBatch* B, const uint64_t* dev_counter_base) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  B->ctr_base = (const unsigned long long*)dev_counter_base;
  return MJL_OK;
}

int mjl_batch_attach_applied(mjlBatch* B, const float* qfrc_applied, const float* xfrc_applied) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  B->qfrc_applied = qfrc_applied;
  B->xfrc_applied = xfrc_applied;
  return MJL_OK;
}

int mjl_env_push(mjlBatch* B, int body, int32_t* timer, int interval_lo, int interval_hi, int duration,
                 float force_lo, float force_hi, const float* done, uint64_t seed, uint64_t counter,
                 const float* noise, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!B->xfrc_applied) return fail(MJL_ERR_ARG, "mjl_env_push needs an attached xfrc_applied");
  if (!timer) return fail(MJL_ERR_ARG, "timer is required");
  const int nbody = B->model->desc.nbody;
  if (body < 1 || body >= nbody) return fail(MJL_ERR_ARG, "body %d outside 1..%d", body, nbody - 1);
  if (interval_lo < 1 || interval_hi < interval_lo) return fail(MJL_ERR_ARG, "need 1 <= interval_lo <= interval_hi");
  if (duration < 1) return fail(MJL_ERR_ARG, "duration must be >= 1");
  HIPCHK(hipSetDevice(B->device));
  PushArgs A;
  A.xfrc = const_cast<float*>(B->xfrc_applied); A.timer = timer; A.done = done; A.noise = noise;
  A.ctr_base = B->ctr_base;
  A.nenv = B->nenv; A.nbody = nbody; A.body = body;
  A.interval_lo = interval_lo; A.interval_hi = interval_hi; A.duration = duration;
  A.force_lo = force_lo; A.force_hi = force_hi;
  A.seed_lo = (uint32_t)seed; A.seed_hi = (uint32_t)(seed >> 32);
  A.ctr_lo = (uint32_t)counter; A.ctr_hi = (uint32_t)(counter >> 32);
  hipLaunchKernelGGL(env_push_kernel, dim3((unsigned)((B->nenv + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_vjp_scale_attach(mjlBatch* B, int32_t* exp, int threshold_log2) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (exp && (threshold_log2 < 0 || threshold_log2 > 96))
    return fail(MJL_ERR_ARG, "threshold_log2 %d outside [0, 96]", threshold_log2);
  if (exp && !B->d_exp_stage) {  // the first attach allocates (outside stream capture); later ones only set pointers
    HIPCHK(hipSetDevice(B->device));
    hipError_t e = hipMalloc(&B->d_exp_stage, (size_t)kExpStage * B->nenv * sizeof(float));
    if (e != hipSuccess) { B->d_exp_stage = nullptr; return fail(MJL_ERR_HIP, "cotangent staging: %s", hipGetErrorString(e)); }
  }
  B->vjp_exp = exp;
  B->vjp_exp_thr = threshold_log2;
  return MJL_OK;
}

int mjl_env_set_reset_keys(mjlBatch* B, const uint32_t* dev_keys, int mode) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (dev_keys && mode != MJL_RNG_JAX_PARTITIONABLE && mode != MJL_RNG_JAX_ORIGINAL)
    return fail(MJL_ERR_ARG, "unknown key mode %d", mode);
  B->reset_keys = dev_keys;
  B->key_mode = mode;
  return MJL_OK;
}

int mjl_env_reset(mjlBatch* B, const float* mask, uint64_t seed, uint64_t counter, const float* noise, float* obs,
                  void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  KParams P = make_params(B);
  P.mask = mask; P.noise = noise; P.obs = obs;
  set_seed_counter(P, seed, counter);
  return launch<MODE_ENV_RESET>(B, P, stream);
}

}  // extern "C"

// ---------------------------------------------------------------- step VJP (APG backward)
// The adjoint of J(q)' w with respect to q is not built: every VJP, record and replay entry checks this
// before anything else, so a batch with applied forces attached is refused whatever the other arguments.
// Nor are the adjoints through per-env model blocks: the same entries refuse a batch with MJL_OPT_PER_ENV_MODEL on.
// Nor is the adjoint of a general actuator's force (its qpos and qvel terms, its clip): a model with any
// non-motor actuator is refused by the same entries, with a message of its own.
static bool applied_attached(const mjlBatch* B) {
  return B && (B->qfrc_applied || B->xfrc_applied || B->d_model_env || B->model->mf.act_general);
}
static int fail_applied(const mjlBatch* B) {
  if (B->model->mf.act_general)
    return fail(MJL_ERR_UNSUPPORTED, "step VJP / record / replay on a model with non-motor (general) actuators: "
                                     "general actuators are not differentiated");
  return fail(MJL_ERR_UNSUPPORTED, "step VJP / record / replay with applied forces attached or per-env model "
                                   "parameters on: detach them (mjl_batch_attach_applied(batch, NULL, NULL)) and "
                                   "set MJL_OPT_PER_ENV_MODEL to 0 first");
}

// The step VJP's per-block scratch (row slab + adjoint scratch): allocated on first use for `blocks` strides and
// regrown when a later call needs more (mjl_step_jacobian with row groups: nenv x groups), so outside stream
// capture. A regrow frees the old buffer: graphs captured against it must be captured again.
static int ensure_adj_scratch(mjlBatch* B, int blocks) {
  if (B->d_adj_scratch && blocks <= B->adj_blocks) return MJL_OK;
  const int LD = B->model->nvc == 0 ? DHum::LD : DGen::LD;
  B->adj_row_floats = row_slab_floats(LD, B->gmax_efc, B->gmax_con);
  B->adj_row_floats = (B->adj_row_floats + 3) & ~3;
  B->adj_stride = B->adj_row_floats + adj_scratch_floats(B->gmax_efc, B->gmax_con);
  if (B->model->nvc == 0) B->adj_stride += DHumV::NV * DHumV::LD;  // lean unrolled replay: M-bar rows
  B->adj_stride = (B->adj_stride + 3) & ~3;
  (void)hipFree(B->d_adj_scratch);
  B->d_adj_scratch = nullptr; B->adj_blocks = 0;
  hipError_t e = hipMalloc(&B->d_adj_scratch, (size_t)B->adj_stride * blocks * sizeof(float));
  if (e != hipSuccess) { B->d_adj_scratch = nullptr; return fail(MJL_ERR_HIP, "adjoint scratch: %s", hipGetErrorString(e)); }
  B->adj_blocks = blocks;
  return MJL_OK;
}

template <bool ENV, int TM = 0> static int launch_vjp(mjlBatch* B, const VjpArgs& V0, void* stream,
                                                     const KParams* P0 = nullptr) {
  HIPCHK(hipSetDevice(B->device));
  if (int rc = ensure_adj_scratch(B, B->nenv)) return rc;
  if (B->vjp_unrolled && !B->d_unr) {
    B->unr_dims.init(B->model->nvc == 0 ? DHum::LD : DGen::LD, B->gmax_efc, B->model->desc.iterations);
    hipError_t e = hipMalloc(&B->d_unr, (size_t)B->unr_dims.stride * B->nenv * sizeof(float));
    if (e != hipSuccess) { B->d_unr = nullptr; return fail(MJL_ERR_HIP, "unrolled VJP tape: %s", hipGetErrorString(e)); }
  }
  KParams P = P0 ? *P0 : make_params(B);
  VjpArgs V = V0;
  V.unr = B->vjp_unrolled ? B->d_unr : nullptr;
  V.slot_stride = B->vt.stride;
  V.s_w = B->vt.w; V.s_a = B->vt.a; V.s_r = B->vt.r; V.s_t = B->vt.t;
  V.td = B->unr_dims;
  V.scratch = B->d_adj_scratch;
  V.scratch_stride = B->adj_stride;
  V.row_floats = B->adj_row_floats;
  if (ENV && TM != 1) { V.exp = B->vjp_exp; V.exp_thr = B->vjp_exp_thr; V.exp_stage = B->d_exp_stage; }
  // one launch of a (KParams, VjpArgs) kernel over the envs; the rest of this function is the table of
  // which kernel runs: lean replay, LDS-row record (+- unrolled), record with its post-step update split
  // off, default
  const auto launch1 = [&](void (*kernel)(KParams, VjpArgs), const VjpArgs& Va) {
    hipLaunchKernelGGL(kernel, dim3(B->nenv), dim3(64), 0, (hipStream_t)stream, P, Va);
    return hipGetLastError();
  };
  const bool hum = B->model->nvc == 0;
  // the replay on the humanoid dims takes the lean layout (20 KB of LDS: one round of 8 envs per CU;
  // MJL_VJP_LEAN=0 keeps the full one, for A/B)
  static const bool lean_ok = [] { const char* e = std::getenv("MJL_VJP_LEAN"); return !(e && e[0] == '0'); }();
  if constexpr (TM == 2) {
    // (unrolled: CG only -- its reverse sweep refactors nothing; Newton's per-iteration Hessian factors
    // need the full layout's LDS)
    if (hum && (!B->vjp_unrolled || B->model->desc.solver == MJL_SOLVER_CG) && lean_ok) {
      HIPCHK(launch1(vjp_kernel<DHumV, ENV, TM, true>, V));
      return MJL_OK;
    }
  }
  // the implicit record on the humanoid dims keeps its rows in LDS (vjp_record_kernel, the same slot as
  // vjp_kernel's record); MJL_OPT_FORCE_GLOBAL_ROWS keeps the global-row record (A/B, parity tests)
  if constexpr (TM == 1 && ENV) {
    if (hum && !B->force_global_rows) {
      HIPCHK(launch1(B->vjp_unrolled ? vjp_record_kernel<DHum, DHumV, true> : vjp_record_kernel<DHum, DHumV>, V));
      return MJL_OK;
    }
    if (V.post.alive) {  // the other record kernels leave the post-step update to its own launch
      VjpArgs V2 = V;
      V2.post.alive = nullptr;
      HIPCHK(launch1(hum ? vjp_kernel<DHumV, ENV, TM> : vjp_kernel<DGen, ENV, TM>, V2));
      hipLaunchKernelGGL(apg_post_kernel, dim3((B->nenv + kPostEnvs - 1) / kPostEnvs), dim3(64 * kPostEnvs), 0,
                         (hipStream_t)stream, B->s, B->model->desc.nq, B->model->desc.nv, P.rew, P.term, P.trunc,
                         V.post);
      HIPCHK(hipGetLastError());
      return MJL_OK;
    }
  }
  HIPCHK(launch1(hum ? vjp_kernel<DHumV, ENV, TM> : vjp_kernel<DGen, ENV, TM>, V));
  return MJL_OK;
}

// the cotangent pointers of a step VJP (null: the entry point has no such input / output)
static VjpArgs vjp_io(const float* act, const float* g_qpos, const float* g_qvel, const float* g_ws, const float* g_rew,
                      const float* g_aux, float* o_qpos, float* o_qvel, float* o_ws, float* o_ctrl, float* o_aux,
                      float* nonfinite) {
  VjpArgs V;
  std::memset(&V, 0, sizeof(V));
  V.act = act; V.g_qpos = g_qpos; V.g_qvel = g_qvel; V.g_rew = g_rew; V.g_aux = g_aux;
  V.o_qpos = o_qpos; V.o_qvel = o_qvel; V.o_ctrl = o_ctrl; V.o_aux = o_aux;
  V.g_ws = g_ws; V.o_ws = o_ws;
  V.nonfinite = nonfinite;
  return V;
}

// tape slot `slot` of the batch, or null with the error set
static float* tape_slot(const mjlBatch* B, int slot) {
  if (!B->d_vtape || slot < 0 || slot >= B->vtape_slots) {
    fail(MJL_ERR_ARG, "VJP tape slot %d not allocated", slot);
    return nullptr;
  }
  return B->d_vtape + (size_t)slot * B->nenv * (size_t)B->vt.stride;
}

// a record launch's arguments: the env step's outputs into P, the action and the (validated, tape_slot)
// slot into the VjpArgs
static VjpArgs record_io(mjlBatch* B, float* slot, const float* act, float* obs, float* rew, float* term, float* trunc,
                         KParams& P) {
  P = make_params(B);
  P.obs = obs; P.rew = rew; P.term = term; P.trunc = trunc;
  VjpArgs V = vjp_io(act, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  V.slot = slot;
  return V;
}

// the env-step VJPs: the recompute (TM 0) or the replay of tape slot `slot` (TM 2)
template <int TM> static int env_vjp(mjlBatch* B, int slot, VjpArgs V, void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !V.act || !V.g_qpos || !V.g_qvel || !V.g_rew || !V.g_aux || !V.o_qpos || !V.o_qvel || !V.o_ctrl || !V.o_aux)
    return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  if (TM == 2 && !(V.slot = tape_slot(B, slot))) return MJL_ERR_ARG;
  return launch_vjp<true, TM>(B, V, stream);
}

extern "C" {

int mjl_step_vjp(mjlBatch* B, const float* g_qpos, const float* g_qvel, float* out_qpos, float* out_qvel,
                 float* out_ctrl, void* stream) {
  return mjl_step_vjp_full(B, g_qpos, g_qvel, nullptr, out_qpos, out_qvel, nullptr, out_ctrl, stream);
}

int mjl_env_step_vjp(mjlBatch* B, const float* act, const float* g_qpos, const float* g_qvel, const float* g_rew,
                     const float* g_aux, float* out_qpos, float* out_qvel, float* out_act, float* out_aux,
                     void* stream) {
  return mjl_env_step_vjp_guarded(B, act, g_qpos, g_qvel, g_rew, g_aux, out_qpos, out_qvel, out_act, out_aux, nullptr,
                                  stream);
}

int mjl_env_step_vjp_guarded(mjlBatch* B, const float* act, const float* g_qpos, const float* g_qvel,
                             const float* g_rew, const float* g_aux, float* out_qpos, float* out_qvel,
                             float* out_act, float* out_aux, float* nonfinite_count, void* stream) {
  return mjl_env_step_vjp_full(B, act, g_qpos, g_qvel, nullptr, g_rew, g_aux, out_qpos, out_qvel, nullptr, out_act,
                               out_aux, nonfinite_count, stream);
}

int mjl_step_vjp_full(mjlBatch* B, const float* g_qpos, const float* g_qvel, const float* g_qacc_ws,
                      float* out_qpos, float* out_qvel, float* out_qacc_ws, float* out_ctrl, void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !g_qpos || !g_qvel || !out_qpos || !out_qvel || !out_ctrl) return fail(MJL_ERR_ARG, "bad argument");
  return launch_vjp<false>(B, vjp_io(nullptr, g_qpos, g_qvel, g_qacc_ws, nullptr, nullptr, out_qpos, out_qvel,
                                     out_qacc_ws, out_ctrl, nullptr, nullptr), stream);
}

// Row groups per env of mjl_step_jacobian: the forward is repeated by every group, so groups pay only while the
// envs alone leave SIMDs idle. The rule and the measurements behind it: DESIGN.md "Linearization",
// profiles/linearize/cost.json.
static int linearize_groups(const mjlBatch* B) {
  if (B->lin_groups > 0) return B->lin_groups;
  int g = B->simds > 0 ? B->simds / B->nenv : 1;
  return g < 1 ? 1 : (g > kLinMaxGroups ? kLinMaxGroups : g);
}

// One launch (linearize_kernels.hip): per (env, row group) the step's forward once, then the implicit VJP's reverse
// passes once per output row.
int mjl_step_jacobian(mjlBatch* B, const float* mask, const float* ctrl, int flags, float* A, float* Bm, void* stream) {
  if (!B) return fail(MJL_ERR_ARG, "null batch");
  if (!A && !Bm) return fail(MJL_ERR_ARG, "mjl_step_jacobian: A and B are both NULL");
  if (flags & ~MJL_JAC_TANGENT) return fail(MJL_ERR_ARG, "mjl_step_jacobian: flags = %d: 0 or MJL_JAC_TANGENT", flags);
  if (applied_attached(B)) return fail_applied(B);
  HIPCHK(hipSetDevice(B->device));
  const int G = linearize_groups(B);
  if ((long long)B->nenv * G > 0x7fffffffLL) return fail(MJL_ERR_ARG, "mjl_step_jacobian: %d envs x %d row groups", B->nenv, G);
  if (int rc = ensure_adj_scratch(B, B->nenv * G)) return rc;
  KParams P = make_params(B);
  LinArgs L;
  L.ctrl = ctrl ? ctrl : B->s.ctrl; L.mask = mask; L.A = A; L.B = Bm;
  L.scratch = B->d_adj_scratch; L.scratch_stride = B->adj_stride; L.row_floats = B->adj_row_floats;
  L.groups = G; L.tangent = (flags & MJL_JAC_TANGENT) != 0;
  if (B->model->nvc == 0)
    hipLaunchKernelGGL(linearize_kernel<DHumV>, dim3(B->nenv * G), dim3(64), 0, (hipStream_t)stream, P, L);
  else
    hipLaunchKernelGGL(linearize_kernel<DGen>, dim3(B->nenv * G), dim3(64), 0, (hipStream_t)stream, P, L);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

int mjl_env_step_vjp_full(mjlBatch* B, const float* act, const float* g_qpos, const float* g_qvel,
                          const float* g_qacc_ws, const float* g_rew, const float* g_aux, float* out_qpos,
                          float* out_qvel, float* out_qacc_ws, float* out_act, float* out_aux,
                          float* nonfinite_count, void* stream) {
  return env_vjp<0>(B, -1, vjp_io(act, g_qpos, g_qvel, g_qacc_ws, g_rew, g_aux, out_qpos, out_qvel, out_qacc_ws, out_act,
                                  out_aux, nonfinite_count), stream);
}

int mjl_env_step_record(mjlBatch* B, int slot, const float* act, float* obs, float* rew, float* term, float* trunc,
                        void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !act || !obs || !rew || !term || !trunc) return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  float* const sp = tape_slot(B, slot);
  if (!sp) return MJL_ERR_ARG;
  KParams P;
  return launch_vjp<true, 1>(B, record_io(B, sp, act, obs, rew, term, trunc, P), stream, &P);
}

int mjl_env_step_record_apg(mjlBatch* B, int slot, const float* act, float* obs, float* rew, float* term, float* trunc,
                            float gamma, float diverge_qvel, uint8_t* alive, float* disc, float* ret, float* dropped,
                            float* grew, float* rfin, void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !act || !obs || !rew || !term || !trunc || !alive || !disc || !ret || !dropped || !grew || !rfin)
    return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  float* const sp = tape_slot(B, slot);
  if (!sp) return MJL_ERR_ARG;
  KParams P;
  VjpArgs V = record_io(B, sp, act, obs, rew, term, trunc, P);
  V.post = ApgPostArgs{gamma, diverge_qvel, alive, disc, ret, dropped, grew, rfin, B->nenv};
  return launch_vjp<true, 1>(B, V, stream, &P);
}

int mjl_env_step_vjp_replay(mjlBatch* B, int slot, const float* act, const float* g_qpos, const float* g_qvel,
                            const float* g_qacc_ws, const float* g_rew, const float* g_aux, float* out_qpos,
                            float* out_qvel, float* out_qacc_ws, float* out_act, float* out_aux,
                            float* nonfinite_count, void* stream) {
  return env_vjp<2>(B, slot, vjp_io(act, g_qpos, g_qvel, g_qacc_ws, g_rew, g_aux, out_qpos, out_qvel, out_qacc_ws,
                                    out_act, out_aux, nonfinite_count), stream);
}

}  // extern "C"

// ---------------------------------------------------------------- PPO host-loop kernels
extern "C" int mjl_gae(const float* rew, const float* val, const float* term, const float* trunc, int T, int B,
                       double gamma, double lam, float* adv, float* ret, void* stream) {
  if (!rew || !val || !term || !trunc || !adv || !ret || T < 0 || B < 0) return fail(MJL_ERR_ARG, "bad argument");
  if (T == 0 || B == 0) return MJL_OK;
  hipLaunchKernelGGL(gae_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, rew, val, term, trunc, T,
                     B, (float)gamma, (float)(gamma * lam), adv, ret);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_obs_normalize(const float* x, const float* mean, const float* var, int n, int dim, float clip,
                                 float* y, void* stream) {
  if (!x || !mean || !var || !y || n < 0 || dim <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (n == 0) return MJL_OK;
  const long long tot = (long long)n * dim;
  hipLaunchKernelGGL(obs_normalize_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x,
                     mean, var, n, dim, clip, y);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_policy_head(const float* z, const float* log_std, const float* eps, int B, int A, float* act,
                               float* logp, void* stream) {
  if (!z || !log_std || !eps || !act || !logp || B < 0 || A <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (B == 0) return MJL_OK;
  hipLaunchKernelGGL(policy_head_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, z, log_std, eps, B,
                     A, act, logp);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

static int policy_dims(int nlayer, const int* dims, PolicyDims& pd) {
  if (nlayer < 1 || nlayer > kPolMaxLayers || !dims) return fail(MJL_ERR_ARG, "policy: 1..%d layers", kPolMaxLayers);
  pd.nlayer = nlayer;
  pd.obs_dim = dims[0];
  pd.act_dim = dims[nlayer];
  long long off = 0;
  for (int l = 0; l < nlayer; l++) {
    if (dims[l] <= 0 || dims[l + 1] <= 0) return fail(MJL_ERR_ARG, "policy: layer sizes must be positive");
    pd.K[l] = (dims[l] + 15) & ~15;
    pd.N[l] = (dims[l + 1] + 15) & ~15;
    if (pd.K[l] > 256 || pd.N[l] > 256) return fail(MJL_ERR_ARG, "policy: layer sizes above 256 not supported");
    pd.off[l] = off;
    off += (long long)pd.K[l] * pd.N[l] + pd.N[l];
  }
  return MJL_OK;
}

extern "C" long long mjl_policy_param_floats(int nlayer, const int* dims) {
  PolicyDims pd;
  if (policy_dims(nlayer, dims, pd) != MJL_OK) return -1;
  const int l = nlayer - 1;
  return pd.off[l] + (long long)pd.K[l] * pd.N[l] + pd.N[l];
}

extern "C" int mjl_policy_fwd(const float* obs, const float* mean, const float* var, float clip, const float* params,
                              int nlayer, const int* dims, const float* log_std, const float* eps, int B, float* act,
                              float* logp, void* stream) {
  if (!obs || !mean || !var || !params || !log_std || !eps || !act || !logp || B < 0)
    return fail(MJL_ERR_ARG, "bad argument");
  PolicyDims pd;
  if (int rc = policy_dims(nlayer, dims, pd)) return rc;
  if (B == 0) return MJL_OK;
  hipLaunchKernelGGL(policy_rollout_kernel, dim3((B + 15) / 16), dim3(64 * kPolWaves), 0, (hipStream_t)stream, obs, mean, var,
                     clip, params, pd, log_std, eps, B, act, logp);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" long long mjl_colsum_scratch(int n, int d) {
  if (n <= 0 || d <= 0) return 0;
  const ColsumPlan p(n, d);
  return p.R > 1 ? (long long)p.R * d : 0;
}

// batched plans (nb > 1): the stage-1 chunks must not straddle two matrices, so n % chunk == 0; the
// stage-2 "chunk" is then one matrix's R / nb chunk rows, and stage 2 writes out[b][d] directly
static int batched_plan_ok(int nb, int n, const ColsumPlan& p) { return nb == 1 || (p.R > 1 && n % p.chunk == 0); }

extern "C" long long mjl_colsum_batched_scratch(int nb, int n, int d) {
  if (nb <= 0 || n <= 0 || d <= 0) return 0;
  const ColsumPlan p(n, d);
  return p.R > 1 ? (long long)nb * p.R * d : 0;
}

// first stages only, with the caller's chunk: partials [nb][n / chunk][d] (the twin update reduces
// every layer's partials together afterwards, mjl_slice_sum_multi; 32-row chunks give its 8,192-row
// minibatch 512 blocks per pass where the two-stage plan's 128-row chunks gave 128 for 256 CUs)
extern "C" int mjl_tanh_bwd_colsum_partials(const float* g, const float* y, int nb, int n, int d, int chunk, float* dz,
                                            float* partials, void* stream) {
  if (!g || !y || !dz || !partials || nb <= 0 || n <= 0 || d <= 0 || chunk <= 0 || n % chunk)
    return fail(MJL_ERR_ARG, "bad argument");
  if (d % 4 || ((uintptr_t)g | (uintptr_t)y | (uintptr_t)dz | (uintptr_t)partials) % 16)
    return fail(MJL_ERR_ARG, "tanh_bwd_colsum_partials: d divisible by 4 and 16-byte aligned rows expected");
  const int dq = d / 4 < 64 ? d / 4 : 64;
  hipLaunchKernelGGL(tanh_bwd_colsum_kernel, dim3((unsigned)((d / 4 + dq - 1) / dq), (unsigned)(n / chunk * nb)),
                     dim3(256), 0, (hipStream_t)stream, g, y, n * nb, d, dq, chunk, dz, partials);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_colsum_batched(const float* x, int nb, int n, int d, float* scratch, float* out, void* stream) {
  if ((!x && n > 0) || !out || nb <= 0 || n < 0 || d <= 0) return fail(MJL_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) {
    HIPCHK(hipMemsetAsync(out, 0, sizeof(float) * (size_t)d * nb, s));
    return MJL_OK;
  }
  const ColsumPlan p(n, d);
  if (!batched_plan_ok(nb, n, p)) return fail(MJL_ERR_ARG, "colsum_batched: n must be a multiple of %d", p.chunk);
  if (p.R > 1 && !scratch) return fail(MJL_ERR_ARG, "colsum needs mjl_colsum_batched_scratch(nb, n, d) floats of scratch");
  const unsigned tiles1 = (unsigned)((d + p.dc1 - 1) / p.dc1);
  hipLaunchKernelGGL(colsum_kernel, dim3(tiles1, (unsigned)(p.R * nb)), dim3(256), 0, s, x, n * nb, d, p.dc1, p.chunk,
                     p.R > 1 ? scratch : out);
  HIPCHK(hipGetLastError());
  if (p.R > 1) {
    const unsigned tiles2 = (unsigned)((d + p.dc2 - 1) / p.dc2);
    hipLaunchKernelGGL(colsum_kernel, dim3(tiles2, (unsigned)nb), dim3(256), 0, s, scratch, p.R * nb, d, p.dc2, p.R,
                       out);
    HIPCHK(hipGetLastError());
  }
  return MJL_OK;
}

extern "C" int mjl_colsum(const float* x, int n, int d, float* scratch, float* out, void* stream) {
  return mjl_colsum_batched(x, 1, n, d, scratch, out, stream);
}

extern "C" int mjl_tanh_bwd_colsum_batched(const float* g, const float* y, int nb, int n, int d, float* dz,
                                           float* scratch, float* colsum_out, void* stream) {
  if (!g || !y || !dz || !colsum_out || nb <= 0 || n <= 0 || d <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (d % 4 || ((uintptr_t)g | (uintptr_t)y | (uintptr_t)dz | (uintptr_t)colsum_out) % 16)
    return fail(MJL_ERR_ARG, "tanh_bwd_colsum: d divisible by 4 and 16-byte aligned rows expected");
  hipStream_t s = (hipStream_t)stream;
  const ColsumPlan p(n, d);
  if (!batched_plan_ok(nb, n, p)) return fail(MJL_ERR_ARG, "tanh_bwd_colsum_batched: n must be a multiple of %d", p.chunk);
  if (p.R > 1 && (!scratch || (uintptr_t)scratch % 16))
    return fail(MJL_ERR_ARG, "tanh_bwd_colsum needs mjl_colsum_batched_scratch(nb, n, d) floats of 16-byte aligned scratch");
  const int dq = d / 4 < 64 ? d / 4 : 64;
  const unsigned tiles1 = (unsigned)((d / 4 + dq - 1) / dq);
  hipLaunchKernelGGL(tanh_bwd_colsum_kernel, dim3(tiles1, (unsigned)(p.R * nb)), dim3(256), 0, s, g, y, n * nb, d, dq,
                     p.chunk, dz, p.R > 1 ? scratch : colsum_out);
  HIPCHK(hipGetLastError());
  if (p.R > 1) {
    const unsigned tiles2 = (unsigned)((d + p.dc2 - 1) / p.dc2);
    hipLaunchKernelGGL(colsum_kernel, dim3(tiles2, (unsigned)nb), dim3(256), 0, s, scratch, p.R * nb, d, p.dc2, p.R,
                       colsum_out);
    HIPCHK(hipGetLastError());
  }
  return MJL_OK;
}

extern "C" int mjl_tanh_bwd_colsum(const float* g, const float* y, int n, int d, float* dz, float* scratch,
                                   float* colsum_out, void* stream) {
  return mjl_tanh_bwd_colsum_batched(g, y, 1, n, d, dz, scratch, colsum_out, stream);
}

extern "C" int mjl_slice_sum_batched(const float* x, int nb, int ns, long long m, float* out, void* stream) {
  if (!x || !out || nb <= 0 || ns <= 0 || m <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (m % 4 || ((uintptr_t)x | (uintptr_t)out) % 16)
    return fail(MJL_ERR_ARG, "slice_sum: slice length divisible by 4 and 16-byte aligned buffers expected");
  const long long q = m / 4;
  hipLaunchKernelGGL(slice_sum_kernel, dim3((unsigned)((q + 255) / 256), (unsigned)nb), dim3(256), 0,
                     (hipStream_t)stream, x, ns, m, out);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_slice_sum_multi(int nseg, const float* const* x, float* const* out, const int* nb, const int* ns,
                                   const long long* m, float* step0, float* step1, int* ctr, void* stream) {
  if (nseg < 1 || nseg > kSliceSegMax || !x || !out || !nb || !ns || !m) return fail(MJL_ERR_ARG, "bad argument");
  SliceSegs sg;
  std::memset(&sg, 0, sizeof(sg));
  sg.nseg = nseg;
  sg.step0 = step0; sg.step1 = step1; sg.ctr = ctr;
  for (int k = 0; k < nseg; k++) {
    if (!x[k] || !out[k] || nb[k] <= 0 || ns[k] <= 0 || m[k] <= 0) return fail(MJL_ERR_ARG, "bad argument");
    sg.x[k] = x[k]; sg.out[k] = out[k]; sg.m[k] = m[k]; sg.ns[k] = ns[k]; sg.nb[k] = nb[k];
    sg.vec[k] = (m[k] % 4 == 0 && ((uintptr_t)x[k] | (uintptr_t)out[k]) % 16 == 0) ? 1 : 0;
    int lanes = 1;  // lanes per output: about 8 slices each, at most a wave
    while (lanes < 64 && ns[k] >= 16 * lanes) lanes *= 2;
    sg.lanes[k] = lanes;
    const long long units = sg.vec[k] ? m[k] / 4 : m[k];
    const long long outs = 256 / lanes;
    const long long blocks = (long long)nb[k] * ((units + outs - 1) / outs);
    if (sg.blk[k] + blocks >= (1LL << 30)) return fail(MJL_ERR_ARG, "slice_sum_multi: too many elements");
    sg.blk[k + 1] = sg.blk[k] + (int)blocks;
  }
  hipLaunchKernelGGL(slice_sum_multi_kernel, dim3((unsigned)sg.blk[nseg]), dim3(256), 0, (hipStream_t)stream, sg);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_slice_sum(const float* x, int ns, long long m, float* out, void* stream) {
  return mjl_slice_sum_batched(x, 1, ns, m, out, stream);
}

extern "C" int mjl_bias_act(float* x, const float* bias, int nb, long long rows, int n, unsigned act_mask,
                            void* stream) {
  if (!x || !bias || nb <= 0 || rows < 0 || n <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (rows == 0) return MJL_OK;
  if ((long long)nb * rows * n >= (1LL << 31)) return fail(MJL_ERR_ARG, "bias_act: at most 2^31 elements");
  const bool v4 = n % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)bias % 16 == 0;
  const long long groups = (long long)nb * rows * n / (v4 ? 4 : 1);
  const dim3 grid((unsigned)((groups + 255) / 256));
  if (v4)
    hipLaunchKernelGGL(bias_act_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, x, bias, nb, rows, n, act_mask);
  else
    hipLaunchKernelGGL(bias_act_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, x, bias, nb, rows, n, act_mask);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_tanh_inplace(float* x, long long n, void* stream) {
  if (!x || n < 0) return fail(MJL_ERR_ARG, "bad argument");
  if (n % 4 || (uintptr_t)x % 16) return fail(MJL_ERR_ARG, "tanh_inplace: length divisible by 4, 16-byte aligned");
  if (n == 0) return MJL_OK;
  const long long q = n / 4;
  hipLaunchKernelGGL(tanh_inplace_kernel, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, q);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// jax.random.split over a batch of keys (train_ppo.py:132,150: random.split(rng); random.split(key, num_envs))
__global__ void prng_split_kernel(const uint32_t* __restrict__ keys, int n, int num, int mode, uint32_t* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * num) return;
  const int k = t / num, j = t % num;
  const uint32_t k0 = keys[2 * (size_t)k], k1 = keys[2 * (size_t)k + 1];
  uint32_t o0, o1;
  if (mode == MJL_RNG_JAX_PARTITIONABLE) {
    o0 = 0u; o1 = (uint32_t)j;
    threefry2x32(k0, k1, o0, o1);
  } else {  // words 2j, 2j + 1 of threefry_2x32(key, iota(2 num)): pairs (c, c + num)
    const uint32_t w0 = (uint32_t)(2 * j), w1 = w0 + 1u, h = (uint32_t)num;
    uint32_t a0 = w0 < h ? w0 : w0 - h, a1 = a0 + h, b0 = w1 < h ? w1 : w1 - h, b1 = b0 + h;
    threefry2x32(k0, k1, a0, a1);
    threefry2x32(k0, k1, b0, b1);
    o0 = w0 < h ? a0 : a1;
    o1 = w1 < h ? b0 : b1;
  }
  out[2 * (size_t)t] = o0;
  out[2 * (size_t)t + 1] = o1;
}

extern "C" int mjl_prng_split(const uint32_t* keys, int n, int num, int mode, uint32_t* out, void* stream) {
  if (!keys || !out || n < 0 || num < 1) return fail(MJL_ERR_ARG, "bad argument");
  if (mode != MJL_RNG_JAX_PARTITIONABLE && mode != MJL_RNG_JAX_ORIGINAL) return fail(MJL_ERR_ARG, "unknown key mode %d", mode);
  if (n == 0) return MJL_OK;
  hipLaunchKernelGGL(prng_split_kernel, dim3((n * num + 255) / 256), dim3(256), 0, (hipStream_t)stream, keys, n, num,
                     mode, out);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// ---------------------------------------------------------------- APG rollout bookkeeping
// U (units per row slot) covers every layer width, and k0 for the backward, whose last layer writes k0
// input cotangents per row (the forward stages its k0 inputs by a loop: 32-unit slots, 8 rows per block,
// for the APG policy's 32-wide layers)
static int small_mlp_setup(int B, int k0, int nl, const int* widths, const float* const* w, const float* const* b,
                           float* const* ys, SmallMlp& P, bool fwd = false) {
  if (B < 0 || nl < 1 || nl > kSmlMaxL || k0 < 1 || k0 > kSmlMaxW || !widths || !w || !b || !ys)
    return fail(MJL_ERR_ARG, "small MLP: 1..%d layers of width 1..%d expected", kSmlMaxL, kSmlMaxW);
  std::memset(&P, 0, sizeof(P));
  P.nl = nl; P.k0 = k0;
  int wmax = fwd ? 1 : k0;
  for (int l = 0; l < nl; l++) {
    if (widths[l] < 1 || widths[l] > kSmlMaxW || !w[l] || !b[l] || !ys[l])
      return fail(MJL_ERR_ARG, "small MLP: layer %d: width 1..%d and non-null pointers expected", l, kSmlMaxW);
    P.n[l] = widths[l]; P.w[l] = w[l]; P.b[l] = b[l]; P.y[l] = ys[l];
    wmax = widths[l] > wmax ? widths[l] : wmax;
  }
  P.u = wmax <= 32 ? 32 : 64;
  return MJL_OK;
}

extern "C" int mjl_small_mlp_fwd(const float* x, int B, int k0, int nl, const int* widths, const float* const* w,
                                 const float* const* b, float* const* ys, void* stream) {
  SmallMlp P;
  int rc = small_mlp_setup(B, k0, nl, widths, w, b, ys, P, true);
  if (rc != MJL_OK) return rc;
  if (!x && B > 0) return fail(MJL_ERR_ARG, "bad argument");
  if (B == 0) return MJL_OK;
  const int R = kSmlThreads / P.u;
  hipLaunchKernelGGL(small_mlp_fwd_kernel<false>, dim3((unsigned)((B + R - 1) / R)), dim3(kSmlThreads), 0,
                     (hipStream_t)stream, x, B, P, ObsIn{});
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_small_mlp_bwd_input(const float* g_out, int B, int k0, int nl, const int* widths,
                                       const float* const* w, const float* const* ys, float* g_x, void* stream) {
  SmallMlp P;
  if (!w || !w[0]) return fail(MJL_ERR_ARG, "bad argument");
  const float* nob[kSmlMaxL] = {w[0], w[0], w[0], w[0]};  // biases unused by the backward
  int rc = small_mlp_setup(B, k0, nl, widths, w, nob, (float* const*)ys, P);
  if (rc != MJL_OK) return rc;
  if ((!g_out || !g_x) && B > 0) return fail(MJL_ERR_ARG, "bad argument");
  if (B == 0) return MJL_OK;
  const int R = kSmlThreads / P.u;
  hipLaunchKernelGGL(small_mlp_bwd_input_kernel<false>, dim3((unsigned)((B + R - 1) / R)), dim3(kSmlThreads), 0,
                     (hipStream_t)stream, g_out, B, P, g_x, ObsVjp{});
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_apg_obs(mjlBatch* B, const uint8_t* alive, const float* mean, const float* var, int use_norm,
                           float* o, float* on, uint8_t* alive_snap, void* stream) {
  if (!B || !alive || !o || !on || !alive_snap || (use_norm && (!mean || !var))) return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  const long n = (long)B->nenv * (nq + nv);
  hipLaunchKernelGGL(apg_obs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B->s,
                     B->nenv, nq, nv, alive, mean, var, use_norm, o, on, alive_snap);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_apg_post(mjlBatch* B, const float* rew, const float* term, const float* trunc, float gamma,
                            float diverge_qvel, uint8_t* alive, float* disc, float* ret, float* dropped, float* grew,
                            float* rfin, void* stream) {
  if (!B || !rew || !term || !trunc || !alive || !disc || !ret || !dropped || !grew || !rfin)
    return fail(MJL_ERR_ARG, "bad argument");
  HIPCHK(hipSetDevice(B->device));
  const ApgPostArgs a{gamma, diverge_qvel, alive, disc, ret, dropped, grew, rfin, B->nenv};
  hipLaunchKernelGGL(apg_post_kernel, dim3((B->nenv + kPostEnvs - 1) / kPostEnvs), dim3(64 * kPostEnvs), 0,
                     (hipStream_t)stream, B->s, B->model->desc.nq, B->model->desc.nv, rew, term, trunc, a);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_apg_obs_vjp(int B, int nq, int nv, const float* o, const uint8_t* alive_snap, const float* mean,
                               const float* var, int use_norm, const float* go, float* g_qpos, float* g_qvel,
                               void* stream) {
  if (B < 0 || nq < 0 || nv < 0 || !o || !alive_snap || !go || !g_qpos || !g_qvel || (use_norm && (!mean || !var)))
    return fail(MJL_ERR_ARG, "bad argument");
  const long n = (long)B * (nq + nv);
  if (n == 0) return MJL_OK;
  hipLaunchKernelGGL(apg_obs_vjp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, B, nq,
                     nv, o, alive_snap, mean, var, use_norm, go, g_qpos, g_qvel);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// mjl_apg_obs then mjl_small_mlp_fwd on its `on`, in one launch (k0 = nq + nv)
extern "C" int mjl_apg_obs_policy_fwd(mjlBatch* B, const uint8_t* alive, const float* mean, const float* var,
                                      int use_norm, float* o, float* on, uint8_t* alive_snap, int nl, const int* widths,
                                      const float* const* w, const float* const* b, float* const* ys, void* stream) {
  if (!B || !alive || !o || !on || !alive_snap || (use_norm && (!mean || !var))) return fail(MJL_ERR_ARG, "bad argument");
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  SmallMlp P;
  int rc = small_mlp_setup(B->nenv, nq + nv, nl, widths, w, b, ys, P, true);
  if (rc != MJL_OK) return rc;
  HIPCHK(hipSetDevice(B->device));
  if (B->nenv == 0) return MJL_OK;
  const ObsIn O{B->s.qpos, B->s.qvel, nq, nv, use_norm, alive, mean, var, o, on, alive_snap};
  const int R = kSmlThreads / P.u;
  hipLaunchKernelGGL(small_mlp_fwd_kernel<true>, dim3((unsigned)((B->nenv + R - 1) / R)), dim3(kSmlThreads), 0,
                     (hipStream_t)stream, nullptr, B->nenv, P, O);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// 1 if this batch's record launch is vjp_record_kernel (the rows in LDS; the post-step update and the next
// step's policy forward can ride along): the humanoid dims, rows not forced global
extern "C" int mjl_env_record_fused(const mjlBatch* B) {
  return B && B->model->nvc == 0 && !B->force_global_rows ? 1 : 0;
}

// the APG record + post-step update + the next step's observation and policy forward, in one launch
extern "C" int mjl_env_step_record_apg_next(mjlBatch* B, int slot, const float* act, float* obs, float* rew, float* term,
                                 float* trunc, float gamma, float diverge_qvel, uint8_t* alive, float* disc, float* ret,
                                 float* dropped, float* grew, float* rfin, const float* mean, const float* var,
                                 int use_norm, float* o, float* on, uint8_t* alive_snap, int nl, const int* widths,
                                 const float* const* w_t, const float* const* b, float* const* ys, void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !act || !obs || !rew || !term || !trunc || !alive || !disc || !ret || !dropped || !grew || !rfin || !o ||
      !on || !alive_snap || (use_norm && (!mean || !var)))
    return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  float* const sp = tape_slot(B, slot);
  if (!sp) return MJL_ERR_ARG;
  if (!mjl_env_record_fused(B)) return fail(MJL_ERR_UNSUPPORTED, "record_apg_next: the humanoid dims' record only");
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  SmallMlp P;
  int rc = small_mlp_setup(B->nenv, nq + nv, nl, widths, w_t, b, ys, P, true);
  if (rc != MJL_OK) return rc;
  KParams Pk;
  VjpArgs V = record_io(B, sp, act, obs, rew, term, trunc, Pk);
  V.post = ApgPostArgs{gamma, diverge_qvel, alive, disc, ret, dropped, grew, rfin, B->nenv};
  V.next = ApgNextArgs{use_norm, mean, var, o, on, alive_snap, P};
  return launch_vjp<true, 1>(B, V, stream, &Pk);
}

// the APG replay with the policy's input backward + the observation's backward added to its state
// cotangents, in one launch
extern "C" int mjl_env_step_vjp_replay_apg(mjlBatch* B, int slot, const float* act, const float* g_qpos,
                                           const float* g_qvel, const float* g_qacc_ws, const float* g_rew,
                                           const float* g_aux, float* out_qpos, float* out_qvel, float* out_qacc_ws,
                                           float* out_act, float* out_aux, float* nonfinite_count, int nl,
                                           const int* widths, const float* const* w, float* const* ys, const float* o,
                                           const uint8_t* alive_snap, const float* mean, const float* var,
                                           int use_norm, void* stream) {
  if (applied_attached(B)) return fail_applied(B);
  if (!B || !act || !g_qpos || !g_qvel || !g_rew || !g_aux || !out_qpos || !out_qvel || !out_act || !out_aux || !o ||
      !alive_snap || !w || !w[0] || (use_norm && (!mean || !var)))
    return fail(MJL_ERR_ARG, "bad argument");
  if (!B->has_env) return fail(MJL_ERR_ARG, "mjl_env_config not called");
  float* const sp = tape_slot(B, slot);
  if (!sp) return MJL_ERR_ARG;
  const int nq = B->model->desc.nq, nv = B->model->desc.nv;
  SmallMlp Pm;
  const float* nob[kSmlMaxL] = {w[0], w[0], w[0], w[0]};  // biases unused by the backward
  int rc = small_mlp_setup(B->nenv, nq + nv, nl, widths, w, nob, ys, Pm);
  if (rc != MJL_OK) return rc;
  if (Pm.n[nl - 1] > 32 || B->model->desc.nu != Pm.n[nl - 1])
    return fail(MJL_ERR_ARG, "replay_apg: the policy's output width must be the action width (<= 32)");
  VjpArgs V = vjp_io(act, g_qpos, g_qvel, g_qacc_ws, g_rew, g_aux, out_qpos, out_qvel, out_qacc_ws, out_act, out_aux,
                     nonfinite_count);
  V.slot = sp;
  V.pbwd = ApgPolicyBwd{use_norm, o, mean, var, alive_snap, Pm};
  return launch_vjp<true, 2>(B, V, stream);
}

// mjl_small_mlp_bwd_input then mjl_apg_obs_vjp on its g_x, in one launch (k0 = nq + nv; g_x not stored)
extern "C" int mjl_apg_policy_bwd_obs_vjp(const float* g_out, int nenv, int nq, int nv, int nl, const int* widths,
                                          const float* const* w, const float* const* ys, const float* o,
                                          const uint8_t* alive_snap, const float* mean, const float* var, int use_norm,
                                          float* g_qpos, float* g_qvel, void* stream) {
  if (!w || !w[0]) return fail(MJL_ERR_ARG, "bad argument");
  if (nenv < 0 || nq < 0 || nv < 0 || ((!g_out || !o || !alive_snap || !g_qpos || !g_qvel) && nenv > 0) ||
      (use_norm && (!mean || !var)))
    return fail(MJL_ERR_ARG, "bad argument");
  SmallMlp P;
  const float* nob[kSmlMaxL] = {w[0], w[0], w[0], w[0]};  // biases unused by the backward
  int rc = small_mlp_setup(nenv, nq + nv, nl, widths, w, nob, (float* const*)ys, P);
  if (rc != MJL_OK) return rc;
  if (nenv == 0) return MJL_OK;
  const ObsVjp O{nq, nv, use_norm, o, alive_snap, mean, var, g_qpos, g_qvel};
  const int R = kSmlThreads / P.u;
  hipLaunchKernelGGL(small_mlp_bwd_input_kernel<true>, dim3((unsigned)((nenv + R - 1) / R)), dim3(kSmlThreads), 0,
                     (hipStream_t)stream, g_out, nenv, P, nullptr, O);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// ---------------------------------------------------------------- PPO update losses
// rows per ppo_surrogate_kernel / twin_loss_head_kernel block (128: 0.2-0.3 ms per C5 per-rank
// update ahead of 64 and 256, profiles/r4/surrogate_rows_ab.txt)
constexpr int kSurrRows = 128;
extern "C" long long mjl_ppo_loss_scratch(int n, int A) {
  if (n <= 0 || A <= 0) return 0;
  const long long nb = (n + kLossT - 1) / kLossT, nbs = (n + kSurrRows - 1) / kSurrRows;
  return 3 * nb + nbs * (A + 1);
}

extern "C" int mjl_ppo_surrogate_clipped(const float* mean, const float* log_std, const float* act,
                                         const float* old_logp, const float* adv, const float* adv_stats,
                                         const int* stats_row, int n, int A, float clip_eps, float ent_coef,
                                         float log_std_lo, float log_std_hi, float* scratch, float* loss,
                                         float* g_mean, float* g_log_std, void* stream) {
  if (!mean || !log_std || !act || !old_logp || !adv || !scratch || !loss || !g_mean || !g_log_std || n <= 0 || A <= 0)
    return fail(MJL_ERR_ARG, "bad argument");
  if (A > kLossMaxA) return fail(MJL_ERR_UNSUPPORTED, "ppo surrogate: at most %d action columns", kLossMaxA);
  hipStream_t s = (hipStream_t)stream;
  const int nb_adv = (n + kLossT - 1) / kLossT, nb = (n + kSurrRows - 1) / kSurrRows;
  float* adv_part = scratch;
  float* part = scratch + 3 * (size_t)nb_adv;
  if (!adv_stats) hipLaunchKernelGGL(adv_stats_kernel, dim3(nb_adv), dim3(kLossT), 0, s, adv, n, adv_part);
  hipLaunchKernelGGL(ppo_surrogate_kernel<kSurrRows>, dim3(nb), dim3(kSurrRows), 0, s, mean, log_std, act, old_logp,
                     adv, n, A, clip_eps, adv_part, nb_adv, adv_stats, g_mean, part, log_std_lo, log_std_hi, stats_row);
  hipLaunchKernelGGL(ppo_surrogate_final_kernel, dim3(A + 1), dim3(64), 0, s, part, nb, n, A, log_std, ent_coef, loss,
                     g_log_std, log_std_lo, log_std_hi);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_ppo_surrogate(const float* mean, const float* log_std, const float* act, const float* old_logp,
                                 const float* adv, const float* adv_stats, int n, int A, float clip_eps,
                                 float ent_coef, float* scratch, float* loss, float* g_mean, float* g_log_std,
                                 void* stream) {
  return mjl_ppo_surrogate_clipped(mean, log_std, act, old_logp, adv, adv_stats, nullptr, n, A, clip_eps, ent_coef,
                                   -INFINITY, INFINITY, scratch, loss, g_mean, g_log_std, stream);
}

// rows per twin loss-head block: 64 at a data-parallel shard's minibatch (8,192 rows: 128 blocks where
// 128-row blocks left 192 of the 256 CUs idle), 128 at C3's 65,536
static int twin_loss_rows(int n) { return n <= 16384 ? 64 : kSurrRows; }
extern "C" long long mjl_twin_loss_head_blocks(int n) {
  return n > 0 ? (n + twin_loss_rows(n) - 1) / twin_loss_rows(n) : 0;
}

extern "C" int mjl_twin_loss_head(const float* z, const float* log_std, const float* act, const float* old_logp,
                                  const float* adv, const float* ret, const float* adv_stats, const int* stats_row,
                                  int n, int A, float clip_eps, float ent_coef, float log_std_lo, float log_std_hi,
                                  const float* bias, float* scratch, float* dz, float* lossp, float* glsp, float* biasp,
                                  void* stream) {
  if (!z || !log_std || !act || !old_logp || !adv || !ret || !scratch || !dz || !lossp || !glsp || !biasp || n <= 0 ||
      A <= 0)
    return fail(MJL_ERR_ARG, "bad argument");
  if (A > kLossMaxA || 2 * A + 2 > 64) return fail(MJL_ERR_UNSUPPORTED, "twin_loss_head: at most %d action columns", 31);
  hipStream_t s = (hipStream_t)stream;
  const int nb_adv = (n + kLossT - 1) / kLossT, nb = (int)mjl_twin_loss_head_blocks(n);
  if (!adv_stats) hipLaunchKernelGGL(adv_stats_kernel, dim3(nb_adv), dim3(kLossT), 0, s, adv, n, scratch);
  if (twin_loss_rows(n) == 64)
    hipLaunchKernelGGL(twin_loss_head_kernel<64>, dim3(nb), dim3(2 * 64), 0, s, z, log_std, act, old_logp, adv,
                       ret, n, A, clip_eps, ent_coef, scratch, nb_adv, adv_stats, stats_row, log_std_lo, log_std_hi, bias,
                       dz, lossp, glsp, biasp);
  else
    hipLaunchKernelGGL(twin_loss_head_kernel<kSurrRows>, dim3(nb), dim3(2 * kSurrRows), 0, s, z, log_std, act, old_logp,
                       adv, ret, n, A, clip_eps, ent_coef, scratch, nb_adv, adv_stats, stats_row, log_std_lo, log_std_hi,
                       bias, dz, lossp, glsp, biasp);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// The twin update's fused thin ends (twin_kernels.hip). Shapes: bit 0 set when the gather + input
// layer launch has an instantiation for (k0, N), bit 1 when the output backward has one for (A, N),
// bit 2 when the fused head (forward + losses + backward) has one for (A, N = the last hidden width).
extern "C" int mjl_twin_fused_shapes(int k0, int A, int N) {
  return (k0 == kTinK0 && N == kTinN ? 1 : 0) | (A == kHbA && N > 0 && N % kHbCols == 0 ? 2 : 0) |
         (A == kThA && N == kThK ? 4 : 0);
}

// workgroups per net of the fused head launch (the partial rows of its reductions): 32-row chunks, two
// workgroups per CU (measured against 64-row chunks with one: 22.8 vs 27.7 us at 8,192 rows, 129.9 vs
// 179.6 us at 65,536; tools/twin_micro.hip)
extern "C" long long mjl_twin_head_blocks(int n) {
  if (n <= 0) return 0;
  const int nchunk = (n + kThRows - 1) / kThRows;
  return nchunk < kThBlocks / 2 ? nchunk : kThBlocks / 2;
}

extern "C" int mjl_twin_head(const float* zh, const float* bh, const float* W, const float* bo, const float* log_std,
                             const float* act, const float* old_logp, const float* adv, const float* ret,
                             const float* adv_stats, const int* stats_row, int n, int A, int K, float clip_eps,
                             float ent_coef, float log_std_lo, float log_std_hi, float* scratch, float* dzh, float* cs,
                             float* gw, float* lossp, float* glsp, float* biasp, void* stream) {
  if (!zh || !bh || !W || !bo || !log_std || !act || !old_logp || !adv || !ret || !dzh || !cs || !gw || !lossp ||
      !glsp || !biasp || n <= 0 || A <= 0 || K <= 0 || (!adv_stats && !scratch))
    return fail(MJL_ERR_ARG, "bad argument");
  if (!(mjl_twin_fused_shapes(0, A, K) & 4))
    return fail(MJL_ERR_UNSUPPORTED, "twin_head: %d outputs / hidden width %d not instantiated", A, K);
  if (n % kThRows) return fail(MJL_ERR_ARG, "twin_head: rows must be a multiple of %d", kThRows);
  if (((uintptr_t)zh | (uintptr_t)bh | (uintptr_t)W | (uintptr_t)dzh) % 16)
    return fail(MJL_ERR_ARG, "twin_head: 16-byte aligned zh, bh, W, dzh expected");
  hipStream_t s = (hipStream_t)stream;
  const int nb_adv = (n + kLossT - 1) / kLossT;
  if (!adv_stats) hipLaunchKernelGGL(adv_stats_kernel, dim3(nb_adv), dim3(kLossT), 0, s, adv, n, scratch);
  TwinHeadArgs p{zh, bh, W, bo, log_std, act, old_logp, adv, ret, adv_stats, stats_row, scratch, nb_adv, n, clip_eps,
                 ent_coef, log_std_lo, log_std_hi, dzh, cs, gw, lossp, glsp, biasp};
  hipLaunchKernelGGL((twin_head_kernel<kThA, kThK, kThRows>), dim3((unsigned)(2 * mjl_twin_head_blocks(n))), dim3(256), 0,
                     s, p);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_twin_gather_in(const long long* idx, const int* idx_row, int n, long long nsrc, int k0, int A,
                                  int N, const float* obs, const float* act, const float* logp, const float* ret,
                                  const float* adv, float* o2, float* a, float* ol, float* r, float* ad,
                                  const float* W, const float* b, float* h, void* stream) {
  if (!idx || !obs || !act || !logp || !ret || !adv || !o2 || !a || !ol || !r || !ad || !W || !b || !h || n <= 0 ||
      nsrc < 0 || A <= 0)
    return fail(MJL_ERR_ARG, "bad argument");
  if (!(mjl_twin_fused_shapes(k0, A, N) & 1))
    return fail(MJL_ERR_UNSUPPORTED, "twin_gather_in: input width %d / hidden width %d not instantiated", k0, N);
  if (((uintptr_t)h | (uintptr_t)b | (uintptr_t)W) % 16)
    return fail(MJL_ERR_ARG, "twin_gather_in: 16-byte aligned h, b and W expected");
  TwinInArgs p{idx, idx_row, n, A, nsrc, obs, act, logp, ret, adv, o2, a, ol, r, ad, W, b, h};
  const int nblk = 2 * ((n + kTinRows - 1) / kTinRows);  // a workgroup per (chunk, net), at most kTinBlocks
  hipLaunchKernelGGL((twin_gather_in_kernel<kTinK0, kTinN>), dim3((unsigned)(nblk < kTinBlocks ? nblk : kTinBlocks)),
                     dim3(kTinN), 0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_twin_head_bwd(const float* dz, const float* W, const float* y, int n, int A, int N, float* dzh,
                                 float* cs, float* gw, void* stream) {
  if (!dz || !W || !y || !dzh || !cs || !gw || n <= 0 || A <= 0 || N <= 0) return fail(MJL_ERR_ARG, "bad argument");
  if (!(mjl_twin_fused_shapes(0, A, N) & 2))
    return fail(MJL_ERR_UNSUPPORTED, "twin_head_bwd: %d outputs / hidden width %d not instantiated", A, N);
  if (n % kHbRows) return fail(MJL_ERR_ARG, "twin_head_bwd: rows must be a multiple of %d", kHbRows);
  if (((uintptr_t)W | (uintptr_t)y | (uintptr_t)dzh | (uintptr_t)cs | (uintptr_t)gw) % 16)
    return fail(MJL_ERR_ARG, "twin_head_bwd: 16-byte aligned buffers expected");
  TwinHeadBwdArgs p{dz, W, y, dzh, cs, gw, n, N};
  hipLaunchKernelGGL(twin_head_bwd_kernel<kHbA>, dim3((unsigned)(n / kHbRows), (unsigned)(N / kHbCols), 2), dim3(256),
                     0, (hipStream_t)stream, p);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_mse_strided(const float* v, int vstride, const float* r, int n, float* scratch, float* loss,
                               float* g_v, void* stream) {
  if (!v || !r || !scratch || !loss || !g_v || n <= 0 || vstride <= 0) return fail(MJL_ERR_ARG, "bad argument");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (n + kLossT - 1) / kLossT;
  hipLaunchKernelGGL(mse_kernel, dim3(nb), dim3(kLossT), 0, s, v, vstride, r, n, g_v, scratch);
  hipLaunchKernelGGL(mse_final_kernel, dim3(1), dim3(64), 0, s, scratch, nb, n, loss);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_mse(const float* v, const float* r, int n, float* scratch, float* loss, float* g_v, void* stream) {
  return mjl_mse_strided(v, 1, r, n, scratch, loss, g_v, stream);
}

extern "C" int mjl_gather_rows_indexed(const long long* idx, const int* idx_row, int n, long long nsrc, int narr,
                                       const float* const* src, float* const* dst, const int* cols, void* stream) {
  if (!idx || n < 0 || nsrc < 0 || narr < 1 || narr > kGatherMax || !src || !dst || !cols)
    return fail(MJL_ERR_ARG, "bad argument");
  GatherArgs g;
  std::memset(&g, 0, sizeof(g));
  g.narr = narr;
  long long tot = 0;
  for (int k = 0; k < narr; k++) {
    if (!src[k] || !dst[k] || cols[k] <= 0) return fail(MJL_ERR_ARG, "bad argument");
    g.src[k] = src[k]; g.dst[k] = dst[k]; g.cols[k] = cols[k];
    tot += cols[k];
  }
  const long long work = (long long)n * tot;
  if (work == 0) return MJL_OK;
  if (work + 255 >= (1ll << 31)) return fail(MJL_ERR_ARG, "gather_rows: rows x total columns must be below 2^31");
  if (tot <= kGatherWaveCols) {
    GatherMap map;
    int q = 0;
    for (int k = 0; k < narr; k++)
      for (int c = 0; c < cols[k]; c++, q++) { map.k[q] = (unsigned char)k; map.c[q] = (unsigned char)c; }
    hipLaunchKernelGGL(gather_rows_wave_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx,
                       n, nsrc, g, map, (int)tot, idx_row);
  } else {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, (hipStream_t)stream, idx,
                       n, nsrc, g, idx_row);
  }
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_gather_rows(const long long* idx, int n, long long nsrc, int narr, const float* const* src,
                               float* const* dst, const int* cols, void* stream) {
  return mjl_gather_rows_indexed(idx, nullptr, n, nsrc, narr, src, dst, cols, stream);
}

static int adam_launch(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                       const long long* numel, float lr, float beta1, float beta2, float eps, int step,
                       const float* step_dev, void* stream) {
  if (nt < 1 || nt > kAdamMaxT || !p || !g || !m || !v || !numel || (!step_dev && step < 1))
    return fail(MJL_ERR_ARG, "bad argument");
  AdamArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nt = nt;
  for (int k = 0; k < nt; k++) {
    if (!p[k] || !m[k] || !v[k] || numel[k] < 0) return fail(MJL_ERR_ARG, "bad argument");
    a.p[k] = p[k]; a.g[k] = g[k]; a.m[k] = m[k]; a.v[k] = v[k];
    a.off[k + 1] = a.off[k] + numel[k];
  }
  if (!step_dev) {
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    a.step_size = lr / bc1;
    a.bc2_sqrt = sqrtf(bc2);
  }
  a.step_dev = step_dev;
  a.lr = lr; a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  const long long n = a.off[nt];
  if (n == 0) return MJL_OK;
  hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

extern "C" int mjl_adam(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                        const long long* numel, float lr, float beta1, float beta2, float eps, int step, void* stream) {
  return adam_launch(nt, p, g, m, v, numel, lr, beta1, beta2, eps, step, nullptr, stream);
}

extern "C" int mjl_adam_dev(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                            const long long* numel, float lr, float beta1, float beta2, float eps, const float* step,
                            void* stream) {
  if (!step) return fail(MJL_ERR_ARG, "bad argument");
  return adam_launch(nt, p, g, m, v, numel, lr, beta1, beta2, eps, 0, step, stream);
}

extern "C" int mjl_adam_multi(int nt, float* const* p, const float* const* g, float* const* m, float* const* v,
                              const long long* numel, const int* group, int ngroups, const float* lr, float beta1,
                              float beta2, float eps, float gscale, float* const* step, int* ctr, int advanced,
                              void* stream) {
  if (nt < 1 || nt > kAdamMultiMaxT || ngroups < 1 || ngroups > kAdamMaxGroups || !p || !g || !m || !v || !numel ||
      !group || !lr || !step)
    return fail(MJL_ERR_ARG, "bad argument");
  AdamMultiArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nt = nt; a.ngroups = ngroups;
  for (int k = 0; k < nt; k++) {
    if (!p[k] || !m[k] || !v[k] || numel[k] < 0 || group[k] < 0 || group[k] >= ngroups)
      return fail(MJL_ERR_ARG, "bad argument");
    a.p[k] = p[k]; a.g[k] = g[k]; a.m[k] = m[k]; a.v[k] = v[k]; a.grp[k] = group[k]; a.numel[k] = numel[k];
    const long long nb = (numel[k] + 255) / 256;
    if ((long long)a.blk[k] + nb >= (1LL << 30)) return fail(MJL_ERR_ARG, "adam_multi: too many elements");
    a.blk[k + 1] = a.blk[k] + (int)nb;
  }
  for (int gi = 0; gi < ngroups; gi++) {
    if (!step[gi]) return fail(MJL_ERR_ARG, "bad argument");
    for (int gj = 0; gj < gi; gj++)
      if (step[gj] == step[gi]) return fail(MJL_ERR_ARG, "adam_multi: groups need distinct step counters");
    a.lr[gi] = lr[gi]; a.step[gi] = step[gi];
  }
  a.b1 = beta1; a.b2 = beta2; a.eps = eps; a.gscale = gscale;
  a.tadd = advanced ? 0.f : 1.f;
  if (a.blk[nt] > 0)
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)a.blk[nt]), dim3(256), 0, (hipStream_t)stream, a);
  if (!advanced)
    hipLaunchKernelGGL(step_counters_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step[0],
                       ngroups > 1 ? step[1] : nullptr, ctr);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}

// ---------------------------------------------------------------------------------------------
// renderer (render_kernels.hip)
// ---------------------------------------------------------------------------------------------
struct mjlRenderer {
  int device, max_frames, nq;
  mjlVisualDesc vis;
  ModelF* d_model;
  RenderConst* d_rc;
  float* d_scene;  // [max_frames, kSceneFloats]
};

extern "C" int mjl_renderer_create(const mjlModel* model, const mjlVisualDesc* vis, int max_frames, int device,
                                   mjlRenderer** out) {
  if (!model || !vis || !out) return fail(MJL_ERR_ARG, "bad argument");
  *out = nullptr;
  const mjlModelDesc& d = model->desc;
  for (int g = 0; g < d.ngeom; g++)
    if (d.geom_type[g] != MJL_GEOM_PLANE && d.geom_type[g] != MJL_GEOM_SPHERE && d.geom_type[g] != MJL_GEOM_CAPSULE)
      return fail(MJL_ERR_UNSUPPORTED, "renderer: geom %d has type %d (plane, sphere and capsule are drawn)", g,
                  d.geom_type[g]);
  if (max_frames < 1 || max_frames > 65535) return fail(MJL_ERR_ARG, "renderer: max_frames must be in 1..65535");
  if (vis->ncam < 0 || vis->ncam > MJL_MAXCAM || vis->checker_geom >= d.ngeom || !(vis->zfar > vis->znear) ||
      !(vis->znear > 0.f))
    return fail(MJL_ERR_ARG, "renderer: bad visual description");
  for (int c = 0; c < vis->ncam; c++)
    if (vis->cam_body[c] < 0 || vis->cam_body[c] >= d.nbody)
      return fail(MJL_ERR_ARG, "renderer: camera %d is on body %d", c, vis->cam_body[c]);
  if (vis->checker_geom >= 0 && (!(vis->checker_cell[0] > 0.f) || !(vis->checker_cell[1] > 0.f)))
    return fail(MJL_ERR_ARG, "renderer: checker cell size must be positive");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MJL_ERR_NOGPU, "no HIP device available");
  if (device < 0 || device >= ndev) return fail(MJL_ERR_ARG, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));
  mjlRenderer* R = new (std::nothrow) mjlRenderer();
  if (!R) return fail(MJL_ERR_ARG, "out of host memory");
  std::memset(R, 0, sizeof(*R));
  R->device = device; R->max_frames = max_frames; R->nq = d.nq; R->vis = *vis;
  RenderConst rc;
  std::memset(&rc, 0, sizeof(rc));
  rc.ngeom = d.ngeom; rc.checker_geom = vis->checker_geom < 0 ? -1 : vis->checker_geom;
  rc.light_directional = vis->light_directional != 0;
  for (int g = 0; g < d.ngeom; g++)
    for (int i = 0; i < 4; i++) rc.geom_rgb[g][i] = vis->geom_rgba[g][i];
  for (int i = 0; i < 3; i++) {
    rc.chk_rgb1[i] = vis->checker_rgb1[i]; rc.chk_rgb2[i] = vis->checker_rgb2[i];
    rc.chk_x[i] = vis->checker_xaxis[i]; rc.chk_y[i] = vis->checker_yaxis[i];
    rc.sky1[i] = vis->sky_rgb1[i]; rc.sky2[i] = vis->sky_rgb2[i];
    rc.light_pos[i] = vis->light_pos[i]; rc.light_dir[i] = vis->light_dir[i];
    rc.diffuse[i] = vis->light_diffuse[i]; rc.ambient[i] = vis->light_ambient[i];
  }
  if (rc.checker_geom >= 0) {
    rc.chk_inv_cell[0] = 1.f / vis->checker_cell[0]; rc.chk_inv_cell[1] = 1.f / vis->checker_cell[1];
  }
  rc.znear = vis->znear; rc.zfar = vis->zfar;
  hipError_t e = hipMalloc(&R->d_model, sizeof(ModelF));
  if (e == hipSuccess) e = hipMemcpy(R->d_model, &model->mf, sizeof(ModelF), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&R->d_rc, sizeof(RenderConst));
  if (e == hipSuccess) e = hipMemcpy(R->d_rc, &rc, sizeof(RenderConst), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(&R->d_scene, (size_t)max_frames * kSceneFloats * sizeof(float));
  if (e != hipSuccess) {
    (void)hipFree(R->d_model); (void)hipFree(R->d_rc); (void)hipFree(R->d_scene);
    delete R;
    return fail(MJL_ERR_HIP, "renderer allocation: %s", hipGetErrorString(e));
  }
  *out = R;
  return MJL_OK;
}

extern "C" void mjl_renderer_destroy(mjlRenderer* R) {
  if (!R) return;
  (void)hipSetDevice(R->device);
  (void)hipFree(R->d_model); (void)hipFree(R->d_rc); (void)hipFree(R->d_scene);
  delete R;
}

extern "C" int mjl_render_qpos(mjlRenderer* R, const float* qpos, int n, int camera, int width, int height, int flags,
                               uint8_t* rgb, float* depth, int32_t* seg, void* stream) {
  if (!R || !qpos) return fail(MJL_ERR_ARG, "bad argument");
  if (n < 1 || n > R->max_frames) return fail(MJL_ERR_ARG, "render: %d frames (the renderer holds 1..%d)", n, R->max_frames);
  if (width < 1 || height < 1 || width > 16384 || height > 16384)
    return fail(MJL_ERR_ARG, "render: size %d x %d (1..16384 each)", width, height);
  if (camera < 0 || camera >= R->vis.ncam) return fail(MJL_ERR_ARG, "render: camera %d of %d", camera, R->vis.ncam);
  if (!rgb && !depth && !seg) return fail(MJL_ERR_ARG, "render: no output requested");
  const mjlVisualDesc& v = R->vis;
  const int mode = v.cam_mode[camera];
  if (mode != MJL_CAM_FIXED && mode != MJL_CAM_TRACK && mode != MJL_CAM_TRACKCOM)
    return fail(MJL_ERR_UNSUPPORTED, "render: camera %d has an unsupported mode", camera);
  if (!(v.cam_fovy[camera] > 0.f && v.cam_fovy[camera] < 180.f))
    return fail(MJL_ERR_ARG, "render: camera %d has fovy %g", camera, (double)v.cam_fovy[camera]);
  RenderCam cam;
  cam.body = v.cam_body[camera]; cam.mode = mode;
  cam.tan_half = (float)std::tan(0.5 * (double)v.cam_fovy[camera] * 3.14159265358979323846 / 180.0);
  const bool fixed = mode == MJL_CAM_FIXED;
  for (int i = 0; i < 3; i++) cam.pos[i] = fixed ? v.cam_pos[camera][i] : v.cam_pos0[camera][i];
  for (int i = 0; i < 9; i++) cam.mat[i] = fixed ? v.cam_mat[camera][i] : v.cam_mat0[camera][i];
  const int tiles_x = (width + 15) / 16, tiles_y = (height + 15) / 16;
  hipLaunchKernelGGL(render_setup_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, R->d_model, R->d_rc, cam,
                     qpos, R->d_scene);
  hipLaunchKernelGGL(render_rays_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n), dim3(256), 0,
                     (hipStream_t)stream, R->d_rc, R->d_scene, cam.tan_half, width, height, tiles_x,
                     (flags & MJL_RENDER_SHADOWS) != 0, rgb, depth, seg);
  HIPCHK(hipGetLastError());
  return MJL_OK;
}
