// Host side of the model block: mjlModelDesc (include/mjx355.h) -> ModelF (model_dev.h).
// Plain C++17, no HIP: capi.hip includes it, and tools/model_host_check.cpp builds it alone with the host
// compiler under the sanitizers. model_build() checks the descriptor first (model_check: what is supported,
// and every field that the build or a kernel uses as an index or a count), then writes the records and the
// flat members straight from the descriptor: one conversion per value, no staging copy; it cannot fail
// after the check.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "model_dev.h"

namespace mjl {

// sets `msg`, returns `code`: `return model_err(msg, MJL_ERR_ARG, "...", ...)`
inline int model_err(std::string& msg, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int model_err(std::string& msg, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  msg = buf;
  return code;
}

inline void q2m_host(const double* q, double* m) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  m[0] = 1 - 2 * (y * y + z * z); m[1] = 2 * (x * y - w * z); m[2] = 2 * (x * z + w * y);
  m[3] = 2 * (x * y + w * z); m[4] = 1 - 2 * (x * x + z * z); m[5] = 2 * (y * z - w * x);
  m[6] = 2 * (x * z - w * y); m[7] = 2 * (y * z + w * x); m[8] = 1 - 2 * (x * x + y * y);
}

// Every reason to refuse a descriptor, before anything is indexed with its fields: sizes, options, then per
// element the supported kinds and every index and count. Each bound is the one its use needs: the arrays the
// build and the kernels index with the field, and the loops they bound with it.
inline int model_check(const mjlModelDesc* d, std::string& msg) {
  // sensordata has one slot per sensor in the kernels' workspace (touch sensors: one value each)
  if (d->nbody > MJL_MAXBODY || d->njnt > MJL_MAXJNT || d->nv > MJL_MAXV || d->nq > MJL_MAXQ ||
      d->ngeom > MJL_MAXGEOM || d->nsite > MJL_MAXSITE || d->nu > MJL_MAXU || d->ntendon > MJL_MAXTENDON ||
      d->npair > MJL_MAXPAIR || d->nsensor > MJL_MAXSENSOR || d->nsensordata > MJL_MAXSENSOR || d->nbody < 2 ||
      d->nv < 1)
    return model_err(msg, MJL_ERR_UNSUPPORTED, "model sizes exceed kernel capacities");
  const struct { const char* name; int n; } counts[] = {
      {"nq", d->nq}, {"nu", d->nu}, {"njnt", d->njnt}, {"ngeom", d->ngeom}, {"nsite", d->nsite},
      {"ntendon", d->ntendon}, {"npair", d->npair}, {"nsensor", d->nsensor}, {"nsensordata", d->nsensordata}};
  for (const auto& c : counts)
    if (c.n < 0) return model_err(msg, MJL_ERR_ARG, "%s = %d is negative", c.name, c.n);
  if (d->nq - 7 + d->nv + 2 > 64) return model_err(msg, MJL_ERR_UNSUPPORTED, "too many reset draws for one wave");
  if (d->solver != MJL_SOLVER_NEWTON && d->solver != MJL_SOLVER_CG)
    return model_err(msg, MJL_ERR_UNSUPPORTED, "solver %d not supported (Newton, CG)", d->solver);
  if (d->integrator != MJL_INT_EULER && d->integrator != MJL_INT_IMPLICITFAST)
    return model_err(msg, MJL_ERR_UNSUPPORTED, "integrator %d not supported (Euler, implicitfast)", d->integrator);

  // `field[i] = v` must lie in [lo, hi)
#define MJL_RANGE(field, i, v, lo, hi)                                                                       \
  do {                                                                                                       \
    if ((v) < (lo) || (v) >= (hi))                                                                           \
      return model_err(msg, MJL_ERR_ARG, "%s[%d] = %d is outside [%d, %d)", field, (int)(i), (int)(v), (int)(lo), \
                       (int)(hi));                                                                           \
  } while (0)
  for (int b = 0; b < d->nbody; b++) {
    if (b > 0) {  // parents come first: every walk up the tree ends at the world
      MJL_RANGE("body_parentid", b, d->body_parentid[b], 0, d->nbody);
      if (d->body_parentid[b] >= b) return model_err(msg, MJL_ERR_ARG, "bodies must be in DFS order");
    }
    MJL_RANGE("body_rootid", b, d->body_rootid[b], 0, d->nbody);
    MJL_RANGE("body_level", b, d->body_level[b], 0, d->nbody);  // the level loops run to the deepest one
    // joints [jntadr, jntadr + jntnum) and dofs [dofadr, dofadr + dofnum); a body without any may say -1
    MJL_RANGE("body_jntnum", b, d->body_jntnum[b], 0, d->njnt + 1);
    MJL_RANGE("body_jntadr", b, d->body_jntadr[b], d->body_jntnum[b] ? 0 : -1, d->njnt - d->body_jntnum[b] + 1);
    MJL_RANGE("body_dofnum", b, d->body_dofnum[b], 0, d->nv + 1);
    MJL_RANGE("body_dofadr", b, d->body_dofadr[b], d->body_dofnum[b] ? 0 : -1, d->nv - d->body_dofnum[b] + 1);
    MJL_RANGE("body_subtree_end", b, d->body_subtree_end[b], b + 1, d->nbody + 1);  // lanes [b, subtree_end)
  }
  for (int j = 0; j < d->njnt; j++) {
    if (d->jnt_type[j] != MJL_JNT_FREE && d->jnt_type[j] != MJL_JNT_HINGE)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "joint type %d not supported", d->jnt_type[j]);
    MJL_RANGE("jnt_bodyid", j, d->jnt_bodyid[j], 1, d->nbody);  // not the world: the body's parent is looked up
    const bool isfree = d->jnt_type[j] == MJL_JNT_FREE;  // 7 qpos entries and 6 dofs; 1 and 1 otherwise
    if (isfree && d->body_jntadr[d->jnt_bodyid[j]] != j)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "free joint must be the first joint of its body");
    if (isfree && d->body_jntnum[d->jnt_bodyid[j]] != 1)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "a body with a free joint must have no other joint");
    MJL_RANGE("jnt_qposadr", j, d->jnt_qposadr[j], 0, d->nq - (isfree ? 7 : 1) + 1);
    MJL_RANGE("jnt_dofadr", j, d->jnt_dofadr[j], 0, d->nv - (isfree ? 6 : 1) + 1);
  }
  for (int k = 0; k < d->nv; k++) {
    MJL_RANGE("dof_bodyid", k, d->dof_bodyid[k], 0, d->nbody);
    MJL_RANGE("dof_jntid", k, d->dof_jntid[k], 0, d->njnt);
    // a free joint's dof is number k - jnt_dofadr of it: 0..5
    const int j = d->dof_jntid[k], k0 = d->jnt_dofadr[j];
    if (k < k0 || k >= k0 + (d->jnt_type[j] == MJL_JNT_FREE ? 6 : 1))
      return model_err(msg, MJL_ERR_ARG, "dof_jntid[%d] = %d: the dof is not one of that joint's (jnt_dofadr %d)", k, j, k0);
    MJL_RANGE("dof_parentid", k, d->dof_parentid[k], -1, k);  // ancestor walks end at -1
  }
  for (int g = 0; g < d->ngeom; g++) MJL_RANGE("geom_bodyid", g, d->geom_bodyid[g], 0, d->nbody);
  for (int p = 0; p < d->npair; p++) {
    MJL_RANGE("pair_geom1", p, d->pair_geom1[p], 0, d->ngeom);
    MJL_RANGE("pair_geom2", p, d->pair_geom2[p], 0, d->ngeom);
    if (d->pair_kind[p] < MJL_COL_PLANE_SPHERE || d->pair_kind[p] > MJL_COL_CAPSULE_CAPSULE)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "collision kind %d not supported", d->pair_kind[p]);
    if (d->pair_condim[p] != 1 && d->pair_condim[p] != 3)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "condim %d not supported", d->pair_condim[p]);
  }
  for (int s = 0; s < d->nsite; s++) MJL_RANGE("site_bodyid", s, d->site_bodyid[s], 0, d->nbody);
  for (int u = 0; u < d->nu; u++) {
    const int j = d->actuator_trnid[u];
    if (j < 0 || j >= d->njnt || d->jnt_type[j] != MJL_JNT_HINGE)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "actuator %d: only hinge joint transmission supported", u);
    if (d->actuator_kind[u] != MJL_ACT_MOTOR && d->actuator_kind[u] != MJL_ACT_GENERAL)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "actuator %d: kind %d not supported (motor, general)", u,
                       d->actuator_kind[u]);
    if (d->actuator_kind[u] != MJL_ACT_GENERAL) continue;  // a motor reads none of the general fields
    const double prm[6] = {d->actuator_gain[u], d->actuator_biasprm[u][0], d->actuator_biasprm[u][1],
                           d->actuator_biasprm[u][2], d->actuator_forcerange[u][0], d->actuator_forcerange[u][1]};
    for (double x : prm)
      if (!std::isfinite(x))
        return model_err(msg, MJL_ERR_ARG, "actuator %d: gain, biasprm and forcerange must be finite", u);
    if (d->actuator_forcelimited[u] && d->actuator_forcerange[u][0] > d->actuator_forcerange[u][1])
      return model_err(msg, MJL_ERR_ARG, "actuator %d: forcerange [%g, %g] is empty", u, d->actuator_forcerange[u][0],
                       d->actuator_forcerange[u][1]);
  }
  for (int t = 0; t < d->ntendon; t++) {
    MJL_RANGE("tendon_num", t, d->tendon_num[t], 0, MJL_MAXTENWRAP + 1);
    MJL_RANGE("tendon_limited", t, d->tendon_limited[t], 0, 2);  // a flag, counted into the row maximum
    for (int w = 0; w < d->tendon_num[t]; w++)
      if (d->tendon_jnt[t][w] < 0 || d->tendon_jnt[t][w] >= d->njnt)
        return model_err(msg, MJL_ERR_ARG, "tendon_jnt[%d][%d] = %d is outside [0, %d)", t, w, d->tendon_jnt[t][w], d->njnt);
  }
  for (int s = 0; s < d->nsensor; s++) {
    if (d->sensor_type[s] != MJL_SENS_TOUCH) return model_err(msg, MJL_ERR_UNSUPPORTED, "sensor type");
    MJL_RANGE("sensor_objid", s, d->sensor_objid[s], 0, d->nsite);  // touch sensors: a site
    MJL_RANGE("sensor_adr", s, d->sensor_adr[s], 0, d->nsensordata);
  }
  // the readout table (mjl_sensors): every entry's type, object and slice of the sensordata row
  if (d->nrsensor < 0 || d->nrsensordata < 0)
    return model_err(msg, MJL_ERR_ARG, "nrsensor = %d / nrsensordata = %d is negative", d->nrsensor, d->nrsensordata);
  if (d->nrsensor > MJL_MAXRSENSOR || d->nrsensordata > MJL_MAXRSENSORDATA)
    return model_err(msg, MJL_ERR_UNSUPPORTED, "readout table exceeds its capacities (%d sensors, %d values)",
                     MJL_MAXRSENSOR, MJL_MAXRSENSORDATA);
  bool used[MJL_MAXRSENSORDATA] = {};
  for (int s = 0; s < d->nrsensor; s++) {
    const int type = d->rsensor_type[s], ot = d->rsensor_objtype[s], id = d->rsensor_objid[s];
    if (type < 0 || type >= MJL_NSENSTYPE)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "rsensor_type[%d] = %d not supported", s, type);
    const int dim = sensor_type_dim(type);
    bool ok_obj;
    switch (type) {
      case MJL_SENS_TOUCH: ok_obj = ot == MJL_OBJ_TOUCH; break;
      case MJL_SENS_JOINTPOS: case MJL_SENS_JOINTVEL: case MJL_SENS_JOINTACTUATORFRC: case MJL_SENS_JOINTLIMITFRC:
        ok_obj = ot == MJL_OBJ_JOINT; break;
      case MJL_SENS_GYRO: case MJL_SENS_VELOCIMETER: case MJL_SENS_ACCELEROMETER: ok_obj = ot == MJL_OBJ_SITE; break;
      case MJL_SENS_ACTUATORFRC: ok_obj = ot == MJL_OBJ_ACTUATOR; break;
      default: ok_obj = ot == MJL_OBJ_XBODY || ot == MJL_OBJ_SITE; break;  // the frame sensors
    }
    if (!ok_obj)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "rsensor_objtype[%d] = %d not supported for sensor type %d", s, ot, type);
    const int nobj = ot == MJL_OBJ_XBODY ? d->nbody : ot == MJL_OBJ_SITE ? d->nsite : ot == MJL_OBJ_JOINT ? d->njnt
                     : ot == MJL_OBJ_ACTUATOR ? d->nu : d->nsensor;
    MJL_RANGE("rsensor_objid", s, id, 0, nobj);
    if (ot == MJL_OBJ_JOINT && d->jnt_type[id] != MJL_JNT_HINGE)
      return model_err(msg, MJL_ERR_UNSUPPORTED, "rsensor %d: a joint sensor on a free joint is not supported", s);
    if (d->rsensor_dim[s] != dim)
      return model_err(msg, MJL_ERR_ARG, "rsensor_dim[%d] = %d: sensor type %d has dim %d", s, d->rsensor_dim[s], type, dim);
    MJL_RANGE("rsensor_adr", s, d->rsensor_adr[s], 0, d->nrsensordata - dim + 1);
    for (int k = d->rsensor_adr[s]; k < d->rsensor_adr[s] + dim; k++) {
      if (used[k]) return model_err(msg, MJL_ERR_ARG, "rsensor_adr[%d] = %d: the slice overlaps another sensor's", s, d->rsensor_adr[s]);
      used[k] = true;
    }
  }
#undef MJL_RANGE
  return MJL_OK;
}

// The readout table's device block (SensorTab, model_dev.h), beside the model block: the table as it stands in
// the descriptor, the stage of each entry, and the site quaternions (ModelF keeps the sites' matrices only).
// `d` has passed model_check.
inline void sensor_tab_build(const mjlModelDesc* d, SensorTab& t) {
  std::memset(&t, 0, sizeof(t));
  t.n = d->nrsensor; t.ndata = d->nrsensordata;
  for (int s = 0; s < d->nrsensor; s++) {
    t.type[s] = d->rsensor_type[s]; t.objtype[s] = d->rsensor_objtype[s]; t.objid[s] = d->rsensor_objid[s];
    t.adr[s] = d->rsensor_adr[s]; t.dim[s] = d->rsensor_dim[s];
    t.stage[s] = sensor_type_stage(d->rsensor_type[s]);
    t.stages |= t.stage[s];
  }
  for (int s = 0; s < d->nsite; s++)
    for (int i = 0; i < 4; i++) t.site_quat[s][i] = (float)d->site_quat[s][i];
}

// body_iquat of every body (BodyTab, model_dev.h): the principal axes of the body-frame tensor body_inertia by
// cyclic Jacobi rotations in double. Convention (MuJoCo's): the moments in descending order along x, y, z of the
// inertial frame, a proper rotation, quaternion with w >= 0. Moments that coincide leave the axes within their
// eigenspace free; the iteration then keeps the body axes where the tensor is already diagonal (moments that
// tie keep their body-frame order). `d` has passed model_check.
inline void body_tab_build(const mjlModelDesc* d, BodyTab& t) {
  std::memset(&t, 0, sizeof(t));
  for (int b = 0; b < MJL_MAXBODY; b++) t.iquat[b][0] = 1.f;
  for (int b = 1; b < d->nbody; b++) {
    const double* in = d->body_inertia[b];
    double A[3][3] = {{in[0], in[3], in[4]}, {in[3], in[1], in[5]}, {in[4], in[5], in[2]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    const double scale = std::fabs(in[0]) + std::fabs(in[1]) + std::fabs(in[2]);
    for (int sweep = 0; sweep < 64; sweep++) {
      if (std::fabs(A[0][1]) + std::fabs(A[0][2]) + std::fabs(A[1][2]) <= 1e-17 * scale) break;
      for (int p = 0; p < 2; p++)
        for (int q = p + 1; q < 3; q++) {
          if (std::fabs(A[p][q]) <= 1e-300) continue;
          const double theta = (A[q][q] - A[p][p]) / (2 * A[p][q]);
          const double tt = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
          const double c = 1 / std::sqrt(tt * tt + 1), s = tt * c;
          for (int k = 0; k < 3; k++) {  // A <- A G, V <- V G
            const double akp = A[k][p], akq = A[k][q], vkp = V[k][p], vkq = V[k][q];
            A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
            V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
          }
          for (int k = 0; k < 3; k++) {  // A <- G' A
            const double apk = A[p][k], aqk = A[q][k];
            A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
          }
        }
    }
    int ord[3] = {0, 1, 2};  // descending moments, ties in body-frame order (insertion sort: stable)
    for (int i = 1; i < 3; i++)
      for (int j = i; j > 0 && A[ord[j]][ord[j]] > A[ord[j - 1]][ord[j - 1]]; j--) { int x = ord[j]; ord[j] = ord[j - 1]; ord[j - 1] = x; }
    double R[3][3];
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) R[i][k] = V[i][ord[k]];
    const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                       R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
    if (det < 0)
      for (int i = 0; i < 3; i++) R[i][2] = -R[i][2];
    double q[4];  // the largest of the four squared components leads (no cancellation)
    const double tr = R[0][0] + R[1][1] + R[2][2];
    if (tr > 0) {
      const double s = 2 * std::sqrt(tr + 1);
      q[0] = 0.25 * s; q[1] = (R[2][1] - R[1][2]) / s; q[2] = (R[0][2] - R[2][0]) / s; q[3] = (R[1][0] - R[0][1]) / s;
    } else {
      const int i = R[0][0] >= R[1][1] && R[0][0] >= R[2][2] ? 0 : (R[1][1] >= R[2][2] ? 1 : 2), j = (i + 1) % 3, k = (i + 2) % 3;
      const double s = 2 * std::sqrt(1 + R[i][i] - R[j][j] - R[k][k]);
      q[0] = (R[k][j] - R[j][k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (R[j][i] + R[i][j]) / s; q[1 + k] = (R[k][i] + R[i][k]) / s;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) * (q[0] < 0 ? -1.0 : 1.0);
    for (int i = 0; i < 4; i++) t.iquat[b][i] = (float)(q[i] / n);
  }
}

// body_dofmask of every body (DynTab, model_dev.h): the dofs of the body and of its ancestors, as model_build
// derives it for the pairs' PairRec.mask1 / mask2. `d` has passed model_check.
inline void dyn_tab_build(const mjlModelDesc* d, DynTab& t) {
  std::memset(&t, 0, sizeof(t));
  for (int b = 1; b < d->nbody; b++)
    for (int bb = b; bb > 0; bb = d->body_parentid[bb])
      for (int k = d->body_dofadr[bb]; k < d->body_dofadr[bb] + d->body_dofnum[bb]; k++) t.body_dofmask[b] |= 1u << k;
}

// Fills `f` (every byte) and the two capacities the row storage is sized with: the most constraint rows and
// the most contacts one env can have. Returns MJL_OK, or an error code with its text in `msg`; `f` then
// holds nothing of use.
inline int model_build(const mjlModelDesc* d, ModelF& f, int& nefc_max, int& ncon_max, std::string& msg) {
  nefc_max = ncon_max = 0;
  if (int rc = model_check(d, msg)) return rc;
  std::memset(&f, 0, sizeof(f));
  f.nq = d->nq; f.nv = d->nv; f.nu = d->nu; f.nbody = d->nbody; f.njnt = d->njnt; f.ngeom = d->ngeom;
  f.nsite = d->nsite; f.ntendon = d->ntendon; f.npair = d->npair; f.nsensor = d->nsensor;
  f.nsensordata = d->nsensordata; f.iterations = d->iterations; f.ls_iterations = d->ls_iterations;
  f.solver = d->solver; f.integrator = d->integrator; f.eulerdamp = d->eulerdamp;
  f.timestep = (float)d->timestep; f.tolerance = (float)d->tolerance; f.ls_tolerance = (float)d->ls_tolerance;
  f.scale = (float)(1.0 / (d->meaninertia * (d->nv > 1 ? d->nv : 1)));
  for (int i = 0; i < 3; i++) f.gravity[i] = (float)d->gravity[i];

  // bodies: the record, the first three hinges, the tree masks
  uint32_t body_dofmask[MJL_MAXBODY] = {};  // bit k set <=> dof k moves body b (ancestor chain): PairRec.mask1/2
  for (int b = 0; b < d->nbody; b++) {
    BodyRec& r = f.brec[b];
    r.parent = d->body_parentid[b]; r.level = d->body_level[b];
    r.jntadr = d->body_jntadr[b]; r.jntnum = d->body_jntnum[b];
    r.dofadr = d->body_dofadr[b]; r.dofnum = d->body_dofnum[b];
    r.subtree_end = d->body_subtree_end[b]; r.rootid = d->body_rootid[b];
    r.isfree = d->body_jntnum[b] > 0 && d->jnt_type[d->body_jntadr[b]] == MJL_JNT_FREE;
    r.qadr = r.isfree ? d->jnt_qposadr[d->body_jntadr[b]] : 0;
    for (int i = 0; i < 3; i++) { r.pos[i] = (float)d->body_pos[b][i]; r.ipos[i] = (float)d->body_ipos[b][i]; }
    for (int i = 0; i < 4; i++) r.quat[i] = (float)d->body_quat[b][i];
    r.mass = (float)d->body_mass[b];
    for (int i = 0; i < 6; i++) r.inertia[i] = (float)d->body_inertia[b][i];
    for (int k = 0; k < 3 && k < d->body_jntnum[b]; k++) {
      const int j = d->body_jntadr[b] + k;
      for (int i = 0; i < 3; i++) {
        f.bhinge[b][k].pos[i] = (float)d->jnt_pos[j][i];
        f.bhinge[b][k].axis[i] = (float)d->jnt_axis[j][i];
      }
    }
    f.body_subtree_end[b] = d->body_subtree_end[b];
    if (d->body_level[b] > f.maxlevel) f.maxlevel = d->body_level[b];
    if (b == 0) continue;
    const int p = d->body_parentid[b];
    if (p == 0) f.root[f.nroot++] = b;
    for (int bb = b; bb > 0; bb = d->body_parentid[bb]) {
      f.body_ancmask[b] |= 1u << bb;
      for (int k = d->body_dofadr[bb]; k < d->body_dofadr[bb] + d->body_dofnum[bb]; k++) body_dofmask[b] |= 1u << k;
    }
    if (p > 0) {
      f.body_childmask[p] |= 1u << b;
      if (!r.isfree) f.body_childmask_nf[p] |= 1u << b;
    }
    float mr = 0.f;  // the same float sum, in the same order, as a loop over the subtree would take
    for (int c = b; c < d->body_subtree_end[b]; c++) mr += (float)d->body_mass[c];
    f.body_rootmass[b] = mr;
  }

  for (int i = 0; i < d->nq; i++) { f.qpos0[i] = (float)d->qpos0[i]; f.qpos_spring[i] = (float)d->qpos_spring[i]; }

  // joints: the record and the limit-row candidate
  for (int j = 0; j < d->njnt; j++) {
    const int b = d->jnt_bodyid[j];
    const bool isfree = d->jnt_type[j] == MJL_JNT_FREE;
    f.body_jgather[isfree ? b : d->body_parentid[b]] |= 1u << j;
    f.jnt_qposadr[j] = d->jnt_qposadr[j];
    JntRec& r = f.jrec[j];
    LimRec& l = f.jlim[j];
    for (int i = 0; i < 3; i++) { r.pos[i] = (float)d->jnt_pos[j][i]; r.axis[i] = (float)d->jnt_axis[j][i]; }
    r.qadr = d->jnt_qposadr[j];
    r.qpos0 = (float)d->qpos0[r.qadr];
    r.body = b; r.parent = d->body_parentid[b];
    r.isfree = isfree; r.dofadr = d->jnt_dofadr[j];
    l.on = d->jnt_limited[j] && d->jnt_type[j] == MJL_JNT_HINGE;
    nefc_max += l.on;
    l.qadr = d->jnt_qposadr[j]; l.dofadr = d->jnt_dofadr[j];
    l.lo = f.jnt_range[j][0] = (float)d->jnt_range[j][0];
    l.hi = f.jnt_range[j][1] = (float)d->jnt_range[j][1];
    l.margin = (float)d->jnt_margin[j];
    l.invweight = (float)d->dof_invweight0[l.dofadr];
    for (int i = 0; i < 2; i++) l.solref[i] = f.jnt_solref[j][i] = (float)d->jnt_solref[j][i];
    for (int i = 0; i < 5; i++) l.solimp[i] = f.jnt_solimp[j][i] = (float)d->jnt_solimp[j][i];
  }

  for (int k = 0; k < d->nv; k++) {
    DofRec& r = f.drec[k];
    const int j = d->dof_jntid[k];
    r.bodyid = d->dof_bodyid[k]; r.jntid = j; r.rootid = d->body_rootid[r.bodyid];
    r.kfree = d->jnt_type[j] == MJL_JNT_FREE ? k - d->jnt_dofadr[j] : -1;
    for (int a = k; a >= 0; a = d->dof_parentid[a]) {  // ancestors-or-self of k; k a descendant-or-self of a
      r.ancmask |= 1u << a;
      f.dof_descmask[a] |= 1u << k;
    }
    r.qadr_spring = d->jnt_type[j] == MJL_JNT_HINGE ? d->jnt_qposadr[j] : -1;
    r.damping = f.dof_damping[k] = (float)d->dof_damping[k];
    f.any_damping |= d->dof_damping[k] > 0;
    r.armature = (float)d->dof_armature[k];
    r.stiffness = (float)d->jnt_stiffness[j];
    r.qpos_spring = r.qadr_spring >= 0 ? (float)d->qpos_spring[r.qadr_spring] : 0.f;
    r.invweight0 = (float)d->dof_invweight0[k];
  }

  // geoms (lanes 0..31 of frec) and sites (lanes 32 + s)
  for (int g = 0; g < d->ngeom; g++) {
    f.geom_type[g] = d->geom_type[g];
    f.body_geommask[d->geom_bodyid[g]] |= 1u << g;
    FrameRec& r = f.frec[g];
    r.body = d->geom_bodyid[g];
    double gm[9];
    q2m_host(d->geom_quat[g], gm);
    for (int i = 0; i < 3; i++) {
      r.pos[i] = (float)d->geom_pos[g][i];
      r.mat[i] = (float)gm[3 * i + 2];  // the local z axis
      f.geom_size[g][i] = (float)d->geom_size[g][i];
    }
  }
  for (int s = 0; s < d->nsite; s++) {
    FrameRec& r = f.frec[kSiteLane + s];
    r.body = f.site_bodyid[s] = d->site_bodyid[s];
    double sm[9];
    q2m_host(d->site_quat[s], sm);
    for (int i = 0; i < 9; i++) r.mat[i] = (float)sm[i];
    for (int i = 0; i < 3; i++) { r.pos[i] = (float)d->site_pos[s][i]; f.site_size[s][i] = (float)d->site_size[s][i]; }
  }

  for (int p = 0; p < d->npair; p++) {
    const int kind = d->pair_kind[p], condim = d->pair_condim[p];
    PairRec& r = f.prec[p];
    r.g1 = d->pair_geom1[p]; r.g2 = d->pair_geom2[p]; r.kind = kind; r.condim = condim;
    r.r1 = (float)d->geom_size[r.g1][0]; r.h1 = (float)d->geom_size[r.g1][1];
    r.r2 = (float)d->geom_size[r.g2][0]; r.h2 = (float)d->geom_size[r.g2][1];
    r.includemargin = (float)(d->pair_margin[p] - d->pair_gap[p]);
    r.mu = (float)d->pair_friction[p][0];
    r.b1 = d->geom_bodyid[r.g1]; r.b2 = d->geom_bodyid[r.g2];
    r.mask1 = body_dofmask[r.b1]; r.mask2 = body_dofmask[r.b2];
    const double tran = d->body_invweight0[r.b1][0] + d->body_invweight0[r.b2][0];
    if (condim == 1) r.invweight = (float)tran;
    else {  // pyramidal: common invweight for every edge (constraint._efc_contact_pyramidal)
      const double mu = d->pair_friction[p][0];
      const double iw = tran + mu * mu * tran;
      r.invweight = (float)(iw * 2 * mu * mu / d->impratio);
    }
    f.pair_solref[p][0] = (float)d->pair_solref[p][0]; f.pair_solref[p][1] = (float)d->pair_solref[p][1];
    for (int i = 0; i < 5; i++) f.pair_solimp[p][i] = (float)d->pair_solimp[p][i];
    const int nc = kind == MJL_COL_PLANE_CAPSULE ? 2 : 1;
    ncon_max += nc;
    nefc_max += nc * (condim == 1 ? 1 : 2 * (condim - 1));
  }

  for (int u = 0; u < d->nu; u++) {
    f.actuator_dof[u] = d->jnt_dofadr[d->actuator_trnid[u]];
    f.actuator_ctrllimited[u] = d->actuator_ctrllimited[u];
    f.actuator_gear[u] = (float)d->actuator_gear[u];
    f.actuator_ctrlrange[u][0] = (float)d->actuator_ctrlrange[u][0];
    f.actuator_ctrlrange[u][1] = (float)d->actuator_ctrlrange[u][1];
    f.act_general |= d->actuator_kind[u] == MJL_ACT_GENERAL;
  }
  // a model with a general actuator runs them all through arec (its motors as gain 1, no bias, no limit);
  // a motor-only model leaves arec zero and never reads it
  for (int u = 0; u < d->nu && f.act_general; u++) {
    ActRec& r = f.arec[u];
    r.qadr = d->jnt_qposadr[d->actuator_trnid[u]];
    r.gain = 1.f;
    if (d->actuator_kind[u] != MJL_ACT_GENERAL) continue;
    r.gain = (float)d->actuator_gain[u];
    r.b0 = (float)d->actuator_biasprm[u][0]; r.b1 = (float)d->actuator_biasprm[u][1];
    r.b2 = (float)d->actuator_biasprm[u][2];
    r.flim = d->actuator_forcelimited[u] != 0;
    r.flo = (float)d->actuator_forcerange[u][0]; r.fhi = (float)d->actuator_forcerange[u][1];
    f.act_b2 |= r.b2 != 0.f;
  }

  for (int t = 0; t < d->ntendon; t++) {
    f.tendon_num[t] = d->tendon_num[t];
    for (int w = 0; w < d->tendon_num[t]; w++) {
      const int j = d->tendon_jnt[t][w];
      f.tendon_qadr[t][w] = d->jnt_qposadr[j];
      f.tendon_dof[t][w] = d->jnt_dofadr[j];
      f.tendon_coef[t][w] = (float)d->tendon_coef[t][w];
    }
    LimRec& l = f.tlim[t];
    l.on = d->tendon_limited[t];
    nefc_max += d->tendon_limited[t];
    l.lo = f.tendon_range[t][0] = (float)d->tendon_range[t][0];
    l.hi = f.tendon_range[t][1] = (float)d->tendon_range[t][1];
    l.margin = (float)d->tendon_margin[t];
    l.invweight = (float)d->tendon_invweight0[t];
    for (int i = 0; i < 2; i++) l.solref[i] = f.tendon_solref[t][i] = (float)d->tendon_solref[t][i];
    for (int i = 0; i < 5; i++) l.solimp[i] = f.tendon_solimp[t][i] = (float)d->tendon_solimp[t][i];
  }

  for (int s = 0; s < d->nsensor; s++) {
    f.sensor_objid[s] = d->sensor_objid[s]; f.sensor_adr[s] = d->sensor_adr[s];
  }
  return MJL_OK;
}

// The staging block of the per-env model builder (model_params_kernel): the two inputs of PairRec.invweight
// above that ModelF does not keep, in double and by the same expressions, so that the kernel's
//   (tran + mu * mu * tran) * 2 * mu * mu / impratio
// rounds to the float model_build stores. `d` has passed model_check (a model that was created).
inline void model_param_stage(const mjlModelDesc* d, ParamStage& s) {
  std::memset(&s, 0, sizeof(s));
  s.impratio = d->impratio;
  for (int p = 0; p < d->npair; p++) {
    const int b1 = d->geom_bodyid[d->pair_geom1[p]], b2 = d->geom_bodyid[d->pair_geom2[p]];
    s.tran[p] = d->body_invweight0[b1][0] + d->body_invweight0[b2][0];
  }
}

// dim of a per-env parameter row (MJL_MP_*), -1 for an unknown id
inline int model_param_dim(const mjlModelDesc* d, int param) {
  switch (param) {
    case MJL_MP_BODY_MASS: return d->nbody;
    case MJL_MP_BODY_INERTIA: return d->nbody * 6;
    case MJL_MP_DOF_DAMPING: case MJL_MP_DOF_ARMATURE: return d->nv;
    case MJL_MP_ACTUATOR_GEAR: return d->nu;
    case MJL_MP_PAIR_FRICTION: return d->npair;
  }
  return -1;
}

}  // namespace mjl
