"""Body-level readout (mjl_body_data / mjx.body_data), the part that needs no GPU: the declaration and its
binding, tests/bodydata_ref.py against the oracle's own arrays, and the momentum balance of the reference."""
import os
import re

import numpy as np
import pytest

import mjx_amd
from mjx_amd import mjcf, mjx
from mjx_amd._header import HEADER
from mjx_amd._lib import MjlError, lib
from oracle import Oracle, state_arrays

import bodydata_ref as br

NENV = 5
ARGS = ["batch", "mask", "xipos", "ximat", "subtree_com", "cinert", "cvel", "subtree_linvel", "subtree_angmom",
        "cfrc_ext", "cfrc_int", "stream"]
# The bound of the balance tests: the largest |cfrc_int[1]| / scale measured here over both models and both
# variants is 5.1e-15 (the oracle's qacc and the constraint forces it reports satisfy the equation of motion to
# rounding, whatever the solver's own tolerance); asserted with a 10x margin.
BALANCE_BOUND = 5.1e-14

# A fixed-base chain: link1 hangs on the world by a hinge; link2 carries two geoms (its centre of mass is off the
# body origin and its principal axes are not the body's: three distinct moments); link3 a rotated capsule.
CHAIN = """
<mujoco model="bd_chain">
  <option timestep="0.005"/>
  <worldbody>
    <geom name="floor" type="plane" size="5 5 0.1"/>
    <body name="link1" pos="0 0 1.5">
      <joint name="j1" type="hinge" axis="0 1 0" pos="0 0 0.05"/>
      <geom name="g1" type="capsule" fromto="0 0 0 0.3 0 0" size="0.04"/>
      <body name="link2" pos="0.3 0 0" quat="0.9 0.1 0.3 -0.2">
        <joint name="j2" type="hinge" axis="1 0 0"/>
        <joint name="j3" type="hinge" axis="0 0 1" pos="0.02 0 0"/>
        <geom name="g2a" type="capsule" fromto="0 0 0 0.2 0.1 0" size="0.03"/>
        <geom name="g2b" type="sphere" pos="0.05 -0.08 0.12" size="0.05"/>
        <body name="link3" pos="0.2 0.1 0">
          <joint name="j4" type="hinge" axis="0 1 1"/>
          <geom name="g3" type="capsule" fromto="0 0 0 0.1 0.1 0.2" size="0.025"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="a1" joint="j1" gear="20"/>
    <motor name="a2" joint="j2" gear="10"/>
    <motor name="a4" joint="j4" gear="5"/>
  </actuator>
</mujoco>
"""


def build_states(m, seed=5):
    """(qpos, qvel, qacc_warmstart, ctrl) x 5, rounded to float32: random joint angles and velocities; envs 0, 2
    and 3 after a fall from a low pelvis (foot and body contacts), envs 1 and 4 raised, as drawn (the tests assert
    the contact counts they need: at least three envs with contacts, at least one without)."""
    rng = np.random.default_rng(seed)
    od = Oracle(m)
    out = []
    for drop, nst in ((0.25, 30), (-0.4, 0), (0.1, 50), (0.3, 60), (-0.6, 0)):
        q = m.qpos0.copy()
        q[7:] += rng.uniform(-0.3, 0.3, m.nq - 7)
        q[2] -= drop
        s = od.new_state(q, rng.uniform(-1, 1, m.nv), ctrl=rng.uniform(-1, 1, m.nu))
        if nst:
            od.rollout(s, rng.uniform(-1, 1, (nst, m.nu)))
        a = state_arrays(m, s)
        out.append((a["qpos"], a["qvel"], a["qacc_warmstart"], rng.uniform(-1, 1, m.nu)))
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def chain_states(m, seed=9):
    rng = np.random.default_rng(seed)
    out = [(m.qpos0 + rng.uniform(-0.8, 0.8, m.nq), rng.uniform(-2, 2, m.nv), np.zeros(m.nv), rng.uniform(-1, 1, m.nu))
           for _ in range(NENV)]
    return [tuple(np.float32(x).astype(np.float64) for x in st) for st in out]


def oracle_forward(m, states):
    """Per state (state_arrays of the oracle's forward pass, its cinert [nbody, 10])."""
    orc = Oracle(m)
    outs = []
    for st in states:
        s = orc.forward(orc.new_state(*st))
        outs.append((state_arrays(m, s), np.array(s.cinert)[:m.nbody]))
    return outs


def test_declared_and_bound():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "mjx355.h")).read()
    proto = re.search(r"int\s+mjl_body_data\s*\((.*?)\)\s*;", text, re.S)
    assert proto, "mjl_body_data is not declared"
    args = re.sub(r"/\*.*?\*/", "", proto.group(1), flags=re.S).split(",")
    assert [a.split()[-1].lstrip("*") for a in args] == ARGS
    assert [a.split()[-1].count("*") + a.split()[-2].count("*") for a in args] == [1] * 12
    ret, name, types = [p for p in HEADER.protos if p[1] == "mjl_body_data"][0]
    assert ret == "int" and types == ["mjlBatch*"] + ["float*"] * 10 + ["void*"]
    fn = lib().mjl_body_data
    assert len(fn.argtypes) == 12
    assert fn(None, None, *([None] * 9), None) == HEADER.enums["MJL_ERR_ARG"]  # a null batch: refused on the host


def test_unknown_field_raises():
    with pytest.raises(MjlError, match="unknown body_data field"):
        mjx.body_data(None, None, fields=("subtree_com", "cacc"))
    assert list(mjx.BODY_FIELDS) == ARGS[2:11]


@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_reference_against_the_oracles_arrays(name):
    m = mjx_amd.load_model(name)
    for (o, cinert), st in zip(oracle_forward(m, build_states(m)), build_states(m)):
        ref = br.body_data(m, o)
        for f, want in (("xipos", o["xipos"]), ("subtree_com", o["subtree_com"]), ("cinert", cinert), ("cvel", o["cvel"])):
            np.testing.assert_allclose(ref[f], want, rtol=1e-9, atol=1e-9 * np.abs(want).max(), err_msg=f)


@pytest.mark.parametrize("applied", [False, True])
@pytest.mark.parametrize("name", mjx_amd.BUILTIN_MODELS)
def test_momentum_balance_of_the_reference(name, applied):
    """The free root's cfrc_int is zero against sum_b |cfrc_ext[b]| + M |g|: bound BALANCE_BOUND above (measured
    5.1e-15 at most, asserted at 10x). `applied`: xfrc_applied = -m_b g on every body, with the oracle running the
    model without gravity (the equivalence of tests/test_applied_gpu.py), so the balance holds only if the
    reference takes the applied rows with the right sign at the right point."""
    m = mjx_amd.load_model(name)
    states = build_states(m)
    mo, xfrc = m, None
    if applied:
        mo = mjx_amd.load_model(name)
        mo.gravity = np.zeros(3)
        xfrc = np.zeros((m.nbody, 6))
        xfrc[1:, :3] = -np.asarray(m.body_mass)[1:, None] * np.asarray(m.gravity)[None, :]
        assert np.abs(xfrc[m.nbody - 1]).max() > 1.0 and int(m.arrays["body_rootid"][m.nbody - 1]) != m.nbody - 1
    outs = oracle_forward(mo, states)
    ncon = [int(o["ncon"]) for o, _ in outs]
    assert sum(n > 0 for n in ncon) >= 3 and min(ncon) == 0, ncon
    # no contact of these states is marginal: a float32 forward pass finds the same contact set
    assert all(np.abs(o["con_dist"]).min() >= 1e-4 for o, _ in outs if o["ncon"]), [o["con_dist"] for o, _ in outs]
    assert int(m.arrays["body_rootid"][1]) == 1 and m.arrays["jnt_type"][0] == mjcf.JNT_FREE
    worst = 0.0
    for o, _ in outs:
        ref = br.body_data(m, o, xfrc)
        worst = max(worst, float(np.abs(ref["cfrc_int"][1]).max()) / br.balance_scale(m, ref))
        assert np.all(ref["cfrc_ext"][0] == 0) and np.all(ref["cfrc_int"][0] == 0)
    print(name, "applied" if applied else "plain", "worst |cfrc_int[1]| / scale:", worst, "ncon", ncon)
    assert worst <= BALANCE_BOUND


def test_chain_model_qualifies():
    """The chain of the GPU test: body_ipos off the origin and principal axes off the body's on link2."""
    m = mjcf.compile_xml_string(CHAIN, "bd_chain")
    b = m.names["body"].index("link2")
    assert np.abs(m.arrays["body_ipos"][b]).max() > 0.02
    t = np.asarray(m.arrays["body_inertia"][b])
    assert np.abs(t[3:]).max() > 0.05 * np.abs(t[:3]).max()
    pm = br.principal_moments(m)[b]
    assert min(pm[0] - pm[1], pm[1] - pm[2]) > 1e-3 * pm[0]
    assert int(m.arrays["body_parentid"][1]) == 0 and m.arrays["jnt_type"][0] == mjcf.JNT_HINGE
