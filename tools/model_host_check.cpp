// Runs the host model build (csrc/model_host.h) alone, without HIP or Python, so that it can run under the
// host compiler's sanitizers (tests/test_model_host.py):
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o model_host_check model_host_check.cpp
//   model_host_check DESC_FILE...
// Each file holds the raw bytes of one mjlModelDesc. One line per file:
//   <file>\trc=<code>\tnefc_max=<n>\tncon_max=<n>\tsizeof_ModelF=<bytes>\tmsg=<text>
//
//   model_host_check --params DESC_FILE...
// The per-env model parameters' host side: per file, model_build on descriptors with the six MJL_MP_* fields
// substituted (three deterministic substitutions, one with every damping zero) and model_param_stage; checks
// that the staged tran / impratio give, by model_build's expression, the PairRec.invweight it stored, that
// body_rootmass, any_damping and both homes of the damping follow the substituted values, and that nothing
// outside the substituted fields' homes differs from the unsubstituted block. One line per file:
//   <file>\tparams=ok|FAILED: <what>
//
//   model_host_check --block DESC_FILE...
// Writes the model block (the raw bytes of ModelF) that model_build makes of each descriptor to <file>.block.
// One line per file:
//   <file>\trc=<code>\tsizeof_ModelF=<bytes>\tmotor_bytes=<offset of ModelF::arec>\tact_general=<0|1>\tact_b2=<0|1>
// Descriptors with general actuators (MJL_ACT_GENERAL) go through every mode like any other: gear has one home
// in the block (the flat actuator_gear), so --params' byte comparison also shows that a substituted gear leaves
// nothing derived behind in the general actuators' records.
//
//   model_host_check --sensors DESC_FILE...
// The readout table's device block (sensor_tab_build) of each accepted descriptor. One line per file:
//   <file>\trc=0\tn=<sensors>\tndata=<values>\tstages=<mask>\tstage=<s0,s1,...>\tsite_quat0=<w,x,y,z of site 0>
// The readout table's validation (types, object ids by object type, dims, slices) is part of model_build, so
// the default mode covers its rejections (tests/test_sensors.py).
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "../mujoco-mjx-lab_amd/csrc/model_host.h"

namespace {

// `d` with its six per-env fields scaled: variant v picks the factors (each value then taken as (double)(float),
// as the library takes a per-env value)
void substitute(mjlModelDesc& d, int v) {
  const auto fl = [](double x) { return (double)(float)x; };
  for (int b = 0; b < d.nbody; b++) {
    const double s = 0.5 + 0.07 * ((b * 5 + v * 3) % 15);
    d.body_mass[b] = fl(d.body_mass[b] * s);
    for (int i = 0; i < 6; i++) d.body_inertia[b][i] = fl(d.body_inertia[b][i] * s);
  }
  for (int k = 0; k < d.nv; k++) {
    d.dof_damping[k] = v == 2 ? 0.0 : fl(d.dof_damping[k] * (0.5 + 0.1 * ((k + v) % 16)));
    d.dof_armature[k] = fl(d.dof_armature[k] * (0.5 + 0.1 * ((k * 3 + v) % 16)));
  }
  for (int u = 0; u < d.nu; u++) d.actuator_gear[u] = fl(d.actuator_gear[u] * (0.7 + 0.04 * ((u + v) % 16)));
  for (int p = 0; p < d.npair; p++) d.pair_friction[p][0] = fl(d.pair_friction[p][0] * (0.3 + 0.08 * ((p + v) % 16)));
}

std::string check_params(const mjlModelDesc& base) {
  std::unique_ptr<mjl::ModelF> f0(new mjl::ModelF), f(new mjl::ModelF), g(new mjl::ModelF);
  std::unique_ptr<mjl::ParamStage> st(new mjl::ParamStage);
  std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
  int nefc = 0, ncon = 0;
  std::string msg;
  if (mjl::model_build(&base, *f0, nefc, ncon, msg)) return "the descriptor is rejected: " + msg;
  mjl::model_param_stage(&base, *st);
  for (int p = 0; p < MJL_NMP; p++)
    if (mjl::model_param_dim(&base, p) < 0) return "model_param_dim of a known id";
  if (mjl::model_param_dim(&base, MJL_NMP) != -1 || mjl::model_param_dim(&base, -1) != -1) return "model_param_dim of an unknown id";
  for (int v = 0; v < 3; v++) {
    *d = base;
    substitute(*d, v);
    if (mjl::model_build(d.get(), *f, nefc, ncon, msg)) return "a substituted descriptor is rejected: " + msg;
    // g: the unsubstituted block patched the way the device builder patches it
    *g = *f0;
    int any = 0;
    for (int b = 0; b < d->nbody; b++) {
      g->brec[b].mass = (float)d->body_mass[b];
      for (int i = 0; i < 6; i++) g->brec[b].inertia[i] = (float)d->body_inertia[b][i];
      if (b == 0) continue;
      float mr = 0.f;
      for (int c = b; c < d->body_subtree_end[b]; c++) mr += (float)d->body_mass[c];
      g->body_rootmass[b] = mr;
    }
    for (int k = 0; k < d->nv; k++) {
      g->drec[k].damping = g->dof_damping[k] = (float)d->dof_damping[k];
      g->drec[k].armature = (float)d->dof_armature[k];
      any |= (float)d->dof_damping[k] > 0.f;
    }
    g->any_damping = any;
    for (int u = 0; u < d->nu; u++) g->actuator_gear[u] = (float)d->actuator_gear[u];
    for (int p = 0; p < d->npair; p++) {
      const double mu = (double)(float)d->pair_friction[p][0], tran = st->tran[p];
      g->prec[p].mu = (float)mu;
      const double iw = tran + mu * mu * tran;
      g->prec[p].invweight = d->pair_condim[p] == 1 ? (float)tran : (float)(iw * 2 * mu * mu / st->impratio);
    }
    if (std::memcmp(g.get(), f.get(), sizeof(mjl::ModelF)) != 0) {
      const unsigned char *a = (const unsigned char*)g.get(), *b = (const unsigned char*)f.get();
      size_t at = 0;
      while (a[at] == b[at]) at++;
      return "variant " + std::to_string(v) + ": the patched block differs from model_build's at byte " + std::to_string(at);
    }
    if (v == 2 && f->any_damping) return "any_damping with every damping zero";
  }
  return "";
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--params") == 0) {
    int bad = 0;
    for (int a = 2; a < argc; a++) {
      std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
      FILE* fp = std::fopen(argv[a], "rb");
      const bool whole = fp && std::fread(d.get(), sizeof(mjlModelDesc), 1, fp) == 1 && std::fgetc(fp) == EOF;
      if (fp) std::fclose(fp);
      if (!whole) {
        std::fprintf(stderr, "%s: not a file of %zu bytes (one mjlModelDesc)\n", argv[a], sizeof(mjlModelDesc));
        return 2;
      }
      const std::string why = check_params(*d);
      bad += !why.empty();
      std::printf("%s\tparams=%s%s\n", argv[a], why.empty() ? "ok" : "FAILED: ", why.c_str());
    }
    return bad ? 1 : 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--block") == 0) {
    for (int a = 2; a < argc; a++) {
      std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
      std::unique_ptr<mjl::ModelF> f(new mjl::ModelF);
      FILE* fp = std::fopen(argv[a], "rb");
      const bool whole = fp && std::fread(d.get(), sizeof(mjlModelDesc), 1, fp) == 1 && std::fgetc(fp) == EOF;
      if (fp) std::fclose(fp);
      if (!whole) {
        std::fprintf(stderr, "%s: not a file of %zu bytes (one mjlModelDesc)\n", argv[a], sizeof(mjlModelDesc));
        return 2;
      }
      int nefc_max = 0, ncon_max = 0;
      std::string msg;
      const int rc = mjl::model_build(d.get(), *f, nefc_max, ncon_max, msg);
      if (rc == MJL_OK) {
        const std::string out = std::string(argv[a]) + ".block";
        FILE* fo = std::fopen(out.c_str(), "wb");
        const bool ok = fo && std::fwrite(f.get(), sizeof(mjl::ModelF), 1, fo) == 1;
        if (fo) std::fclose(fo);
        if (!ok) {
          std::fprintf(stderr, "%s: cannot write\n", out.c_str());
          return 2;
        }
      }
      std::printf("%s\trc=%d\tsizeof_ModelF=%zu\tmotor_bytes=%zu\tact_general=%d\tact_b2=%d\n", argv[a], rc,
                  sizeof(mjl::ModelF), offsetof(mjl::ModelF, arec), rc ? 0 : f->act_general, rc ? 0 : f->act_b2);
    }
    return 0;
  }
  if (argc > 1 && std::strcmp(argv[1], "--sensors") == 0) {
    for (int a = 2; a < argc; a++) {
      std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
      std::unique_ptr<mjl::ModelF> f(new mjl::ModelF);
      std::unique_ptr<mjl::SensorTab> t(new mjl::SensorTab);
      FILE* fp = std::fopen(argv[a], "rb");
      const bool whole = fp && std::fread(d.get(), sizeof(mjlModelDesc), 1, fp) == 1 && std::fgetc(fp) == EOF;
      if (fp) std::fclose(fp);
      if (!whole) {
        std::fprintf(stderr, "%s: not a file of %zu bytes (one mjlModelDesc)\n", argv[a], sizeof(mjlModelDesc));
        return 2;
      }
      int nefc_max = 0, ncon_max = 0;
      std::string msg;
      const int rc = mjl::model_build(d.get(), *f, nefc_max, ncon_max, msg);
      if (rc != MJL_OK) {
        std::printf("%s\trc=%d\n", argv[a], rc);
        continue;
      }
      mjl::sensor_tab_build(d.get(), *t);
      std::printf("%s\trc=0\tn=%d\tndata=%d\tstages=%d\tstage=", argv[a], t->n, t->ndata, t->stages);
      for (int s = 0; s < t->n; s++) std::printf("%s%d", s ? "," : "", t->stage[s]);
      std::printf("\tsite_quat0=%g,%g,%g,%g\n", t->site_quat[0][0], t->site_quat[0][1], t->site_quat[0][2], t->site_quat[0][3]);
    }
    return 0;
  }
  for (int a = 1; a < argc; a++) {
    // on the heap, exactly sized: the sanitizer sees any read or write past either struct
    std::unique_ptr<mjlModelDesc> d(new mjlModelDesc);
    std::unique_ptr<mjl::ModelF> f(new mjl::ModelF);
    FILE* fp = std::fopen(argv[a], "rb");
    const bool whole = fp && std::fread(d.get(), sizeof(mjlModelDesc), 1, fp) == 1 && std::fgetc(fp) == EOF;
    if (fp) std::fclose(fp);
    if (!whole) {
      std::fprintf(stderr, "%s: not a file of %zu bytes (one mjlModelDesc)\n", argv[a], sizeof(mjlModelDesc));
      return 2;
    }
    int nefc_max = 0, ncon_max = 0;
    std::string msg;
    const int rc = mjl::model_build(d.get(), *f, nefc_max, ncon_max, msg);
    std::printf("%s\trc=%d\tnefc_max=%d\tncon_max=%d\tsizeof_ModelF=%zu\tmsg=%s\n", argv[a], rc, nefc_max, ncon_max,
                sizeof(mjl::ModelF), msg.c_str());
  }
  return 0;
}
