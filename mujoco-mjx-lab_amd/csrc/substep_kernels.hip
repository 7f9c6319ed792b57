// Physics substeps (mjl_step_n / mjl_env_step_n). The entries issue nstep single-step launches from the host: a
// fused kernel (one launch keeping each env in LDS for all substeps, the phases of step_kernels.hip in a
// wave-uniform loop) gave the same bits but measured 0 to 27 % slower than the launches it replaced at 2048 and
// 4096 envs (profiles/substeps/substep_cost.json, DESIGN.md section 3 "Substeps"), so it was dropped. What is
// left here is the env step's control for the plain steps that precede its last substep.
#pragma once

namespace mjl {

// ctrl[e] = clip(flip ? act[e][act_perm] * act_sign : act[e], -1, 1), flip = aux[e][0] > 0.5: the expression of
// load_step_state (envs.py:335-344), so the stored control is bit for bit the one mjl_env_step applies.
__global__ void env_ctrl_kernel(const mjlEnvConfig* cfg, const float* act, const float* aux, float* ctrl, int nenv,
                                int nu) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nenv * nu) return;
  const int e = i / nu, u = i - e * nu;
  const bool flip = aux[(size_t)e * MJL_AUX_DIM] > 0.5f;
  const float a = flip ? act[(size_t)e * nu + cfg->act_perm[u]] * cfg->act_sign[u] : act[i];
  ctrl[i] = fminf(fmaxf(a, -1.f), 1.f);
}

}  // namespace mjl
