"""The host model build (csrc/model_host.h) alone, under the host compiler's address and undefined-behaviour
sanitizers: tools/model_host_check.cpp runs it over the two humanoids and over one mutated descriptor per
rejection, and every result equals what mjl_model_create returns for the same descriptor through ctypes.
Nothing here is loaded into Python with a sanitizer and nothing touches a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import mjx_amd
from mjx_amd import _lib, abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, 1, 2
HUGE = 2**31 - 1


def _set(name, value, *idx):
    def mutate(d):
        if not idx:
            setattr(d, name, value)
        elif len(idx) == 1:
            getattr(d, name)[idx[0]] = value
        else:
            getattr(d, name)[idx[0]][idx[1]] = value
    return mutate


def _both(*ms):
    def mutate(d):
        for m in ms:
            m(d)
    return mutate


# humanoid_mjx: 17 bodies, 22 joints (joint 0 free on body 1; body 3 has the hinges 1 and 2), nq 28, nv 27, 20 geoms,
# 2 sites, 2 tendons of 2 joints, 2 touch sensors. (case, mutation, code, fragment of the message)
REJECTED = [
    # what mjl_model_create has always refused
    ("nbody_over", _set("nbody", abi.MAXBODY + 1), UNSUPPORTED, "model sizes exceed kernel capacities"),
    ("npair_over", _set("npair", abi.MAXPAIR + 1), UNSUPPORTED, "model sizes exceed kernel capacities"),
    ("nbody_one", _set("nbody", 1), UNSUPPORTED, "model sizes exceed kernel capacities"),
    ("reset_draws", _both(_set("nq", abi.MAXQ), _set("nv", abi.MAXV)), UNSUPPORTED, "too many reset draws"),
    ("solver", _set("solver", 0), UNSUPPORTED, "solver 0 not supported"),
    ("integrator", _set("integrator", 1), UNSUPPORTED, "integrator 1 not supported"),
    ("jnt_type", _set("jnt_type", 2, 5), UNSUPPORTED, "joint type 2 not supported"),
    ("free_not_first", _set("jnt_type", 0, 2), UNSUPPORTED, "free joint must be the first joint of its body"),
    ("free_sibling", _set("jnt_type", 0, 1), UNSUPPORTED, "a body with a free joint must have no other joint"),
    ("pair_kind", _set("pair_kind", 5, 0), UNSUPPORTED, "collision kind 5 not supported"),
    ("pair_condim", _set("pair_condim", 4, 0), UNSUPPORTED, "condim 4 not supported"),
    ("actuator_free", _set("actuator_trnid", 0, 0), UNSUPPORTED, "actuator 0: only hinge joint transmission"),
    ("actuator_neg", _set("actuator_trnid", -1, 3), UNSUPPORTED, "actuator 3: only hinge joint transmission"),
    ("actuator_huge", _set("actuator_trnid", HUGE, 3), UNSUPPORTED, "actuator 3: only hinge joint transmission"),
    ("sensor_type", _set("sensor_type", 1, 1), UNSUPPORTED, "sensor type"),
    ("dfs_order", _set("body_parentid", 5, 3), ARG, "bodies must be in DFS order"),
    # counts
    ("nsensordata_over", _set("nsensordata", abi.MAXSENSOR + 1), UNSUPPORTED, "model sizes exceed kernel capacities"),
] + [(f"{n}_neg", _set(n, -1), ARG, f"{n} = -1")
     for n in ("nq", "nu", "njnt", "ngeom", "nsite", "ntendon", "npair", "nsensor", "nsensordata")]

# every index and count of the descriptor: (field, index, values out of range); -1 and a huge value for each
# (-2 where -1 is a value), and the first value past each end that the field's use sets
_OUT_OF_RANGE = [
    ("body_parentid", (3,), (-1, HUGE, 17)),
    ("body_rootid", (3,), (-1, HUGE, 17)),
    ("body_level", (3,), (-1, HUGE, 17)),
    ("body_jntadr", (3,), (-1, HUGE, 21)),  # 2 joints from 21 on: past njnt = 22
    ("body_jntadr", (2,), (-2, HUGE, 23)),  # no joints: -1 is allowed
    ("body_jntnum", (3,), (-1, HUGE, 23)),
    ("body_dofadr", (3,), (-1, HUGE, 26)),  # 2 dofs from 26 on: past nv = 27
    ("body_dofnum", (3,), (-1, HUGE, 28)),
    ("body_subtree_end", (3,), (-1, HUGE, 3, 18)),  # lanes [3, end): at least 4, at most nbody
    ("jnt_bodyid", (5,), (-1, HUGE, 0, 17)),
    ("jnt_qposadr", (5,), (-1, HUGE, 28)),
    ("jnt_qposadr", (0,), (-1, HUGE, 22)),  # a free joint needs 7 entries: 21 is the last address
    ("jnt_dofadr", (5,), (-1, HUGE, 27)),
    ("jnt_dofadr", (0,), (-1, HUGE, 22)),  # a free joint has 6 dofs: 21 is the last address
    ("dof_bodyid", (7,), (-1, HUGE, 17)),
    ("dof_jntid", (7,), (-1, HUGE, 22, 3)),  # joint 3 is a joint, of another dof
    ("dof_jntid", (6,), (0,)),  # the free joint has dofs 0..5
    ("dof_parentid", (7,), (-2, HUGE, 7)),
    ("dof_parentid", (0,), (-2, HUGE, 0)),
    ("geom_bodyid", (2,), (-1, HUGE, 17)),
    ("pair_geom1", (0,), (-1, HUGE, 20)),
    ("pair_geom2", (107,), (-1, HUGE, 20)),
    ("site_bodyid", (1,), (-1, HUGE, 17)),
    ("tendon_num", (0,), (-1, HUGE, abi.MAXTENWRAP + 1)),
    ("tendon_jnt", (1, 1), (-1, HUGE, 22)),
    ("tendon_limited", (1,), (-1, HUGE, 2)),
    ("sensor_objid", (0,), (-1, HUGE, 2)),
    ("sensor_adr", (1,), (-1, HUGE, 2)),
]
for _f, _i, _vals in _OUT_OF_RANGE:
    _at = "".join(f"[{i}]" for i in _i)
    REJECTED += [(f"{_f}{_at}_{v}", _set(_f, v, *_i), ARG, f"{_f}{_at} = {v}") for v in _vals]

# the fields the validation pass must cover
_FIELDS = {"body_parentid", "body_rootid", "body_jntadr", "body_jntnum", "body_dofadr", "body_dofnum",
           "body_subtree_end", "jnt_bodyid", "jnt_qposadr", "jnt_dofadr", "dof_bodyid", "dof_jntid", "dof_parentid",
           "geom_bodyid", "pair_geom1", "pair_geom2", "site_bodyid", "tendon_num", "tendon_jnt", "sensor_objid",
           "sensor_adr"}
assert _FIELDS <= {f for f, _, _ in _OUT_OF_RANGE}
assert len({c[0] for c in REJECTED}) == len(REJECTED)


def _compiler():
    for cxx in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    return None


def _create(L, d):
    """(code, message, nefc_max, ncon_max) of mjl_model_create for one descriptor."""
    h = C.c_void_p()
    rc = L.mjl_model_create(C.byref(d), C.byref(h))
    if rc != OK:
        assert not h.value
        return rc, L.mjl_last_error().decode(), 0, 0
    out = (rc, "", L.mjl_model_nefc_max(h), L.mjl_model_ncon_max(h))
    L.mjl_model_destroy(h)
    return out


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """Per case: what the sanitized stand-alone program printed, and what the library returned."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    tmp = tmp_path_factory.mktemp("model_host")
    exe = tmp / "model_host_check"
    cc = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o",
                         str(exe), os.path.join(ROOT, "tools", "model_host_check.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    L = _lib.lib()
    cases = {}
    for name in ("humanoid", "humanoid_mjx"):
        cases[name] = abi.model_desc(mjx_amd.load_model(name))
    base = bytes(cases["humanoid_mjx"])
    for case, mutate, _, _ in REJECTED:
        cases[case] = abi.ModelDesc.from_buffer_copy(base)
        mutate(cases[case])
    files = []
    for case, d in cases.items():
        files.append(str(tmp / (case + ".desc")))
        with open(files[-1], "wb") as fh:
            fh.write(bytes(d))
    run = subprocess.run([str(exe)] + files, capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", run.stderr[-4000:]  # a clean sanitizer exit
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    out = {}
    for (case, d), path, line in zip(cases.items(), files, lines):
        col = line.split("\t")
        assert col[0] == path and [c.split("=")[0] for c in col[1:]] == ["rc", "nefc_max", "ncon_max", "sizeof_ModelF", "msg"]
        rc, nefc, ncon, size = (int(c.split("=", 1)[1]) for c in col[1:5])
        out[case] = {"alone": (rc, col[5].split("=", 1)[1], nefc, ncon), "lib": _create(L, d), "size": size}
    return out


def test_humanoids_accepted_with_their_maxima(results):
    assert results["humanoid_mjx"]["alone"] == (OK, "", 16 * 4 + 100 + 21 + 2, 116)  # nefc <= 187
    assert results["humanoid"]["alone"] == (OK, "", 303, 175)
    for name in ("humanoid", "humanoid_mjx"):
        assert results[name]["lib"] == results[name]["alone"]
    # one model block, far smaller than the descriptor it is built from
    assert len({r["size"] for r in results.values()}) == 1 and 0 < results["humanoid"]["size"] < abi.desc_size()


@pytest.mark.parametrize("case,code,fragment", [(c, code, frag) for c, _, code, frag in REJECTED])
def test_rejected_alike_alone_and_in_the_library(results, case, code, fragment):
    r = results[case]
    assert r["alone"][0] == code and fragment in r["alone"][1], r["alone"]
    assert r["lib"] == r["alone"]
    assert r["alone"][2:] == (0, 0)
