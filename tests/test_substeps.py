"""Physics substeps (mjl_step_n / mjl_env_step_n), the parts that need no GPU: the binding, the argument checks
of the C entries and the Python API, and the choice of the GPU cases on the float64 oracle."""
import types

import pytest

import mjx_amd
from mjx_amd import abi, apg, mjx
from mjx_amd._lib import MjlError, lib
from mjx_amd.config import reference_ppo_config
from mjx_amd.envs import HumanoidEnv

import substeps_cases as sc


def test_binding_exposes_the_substep_entries():
    assert abi.MAXSUBSTEP == 64
    L = lib()
    assert len(L.mjl_step_n.argtypes) == 4 and len(L.mjl_env_step_n.argtypes) == 11


def test_null_batch_is_an_argument_error():
    L = lib()
    assert L.mjl_step_n(None, None, 2, None) == 1  # MJL_ERR_ARG
    assert L.mjl_env_step_n(None, None, 2, None, None, None, None, 0, 0, 0, None) == 1


@pytest.mark.parametrize("k", [0, -1, 65])
def test_python_api_rejects_counts_outside_the_range(k):
    m = mjx_amd.load_model("humanoid_mjx")
    with pytest.raises(MjlError, match="nstep"):
        mjx.step(None, None, None, nstep=k)  # checked before the batch is touched
    with pytest.raises(MjlError, match="n_frames"):
        HumanoidEnv(types.SimpleNamespace(m=m, nq=m.nq, nv=m.nv, nu=m.nu), reference_ppo_config().env_config, 4,
                    n_frames=k)


def test_apg_env_refuses_substeps():
    env = types.SimpleNamespace(n_frames=2)
    with pytest.raises(ValueError, match="n_frames"):
        apg.HumanoidAPGEnv(env, "implicit")


@pytest.mark.parametrize("name,nsteps", [("humanoid_mjx", (2, 3, 4, 5)), ("humanoid", (3,)), ("tail", (3,))])
def test_gpu_cases_have_contacts_that_change(name, nsteps):
    """So that the GPU comparisons cannot pass vacuously: in every case (model, nstep) at least half of the envs
    have an active contact in every substep, and at least one env's contact count changes between substeps."""
    n = sc.contact_counts(name)
    for k in nsteps:
        c = n[:, :k]
        assert (c.min(axis=1) >= 1).sum() * 2 >= sc.B, (name, k, c.tolist())
        assert (c.max(axis=1) != c.min(axis=1)).any(), (name, k, c.tolist())
