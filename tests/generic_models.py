"""Small models on both sides of the kernel dispatch rule of mjl_model_create (csrc/capi.hip): the humanoid
instantiation DHum serves nv <= 27, nbody <= 17, njnt <= 22, ngeom <= 20, the generic one DGen everything else
within the MJL_MAX* capacities. Every model is MJCF text compiled by mjx_amd.mjcf.

  tail, tail_euler   the golden humanoids plus a three-link tail on the pelvis: every dim over the DHum limit
  nv_only(n)         two free roots with n hinged limb links: n = 16 crosses nv alone, n = 15 sits at nv = 27
  nbody_only(n)      a free root and n chained bodies, every second one welded: 16 crosses nbody alone (18)
  njnt_only(n)       n hinges, two per body, on a fixed binary tree: 23 crosses njnt alone, 22 sits at it
  ngeom_only(n)      one free body carrying n spheres over a plane: 21 crosses ngeom alone (22), 19 sits at 20
  full               nv 32, nbody 32, ngeom 32, npair near 256: a five-limbed tree with rotated body / geom
                     frames, oblique capsules (off-diagonal inertias), joint pos offsets, two joints on one body

MODELS maps a name to (builder, generic?) for the tests."""
import os
import xml.etree.ElementTree as ET

import numpy as np

from mjx_amd import abi, mjcf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DHUM = {"nv": 27, "nbody": 17, "njnt": 22, "ngeom": 20}  # Dims<27, 17, 22, 20, ...> of csrc/step_kernels.hip


def is_generic(m) -> bool:
    """mjl_model_create's rule, restated: any one dim past the humanoid's selects the generic kernels."""
    return not (m.nv <= DHUM["nv"] and m.nbody <= DHUM["nbody"] and m.njnt <= DHUM["njnt"] and m.ngeom <= DHUM["ngeom"])


def over(m) -> set:
    """The dims of m that are past the humanoid instantiation's."""
    return {k for k, lim in DHUM.items() if getattr(m, k) > lim}


def within_capacities(m) -> bool:
    return (m.nv <= abi.MAXV and m.nq <= abi.MAXQ and m.nbody <= abi.MAXBODY and m.njnt <= abi.MAXJNT and
            m.ngeom <= abi.MAXGEOM and m.npair <= abi.MAXPAIR and m.nu <= abi.MAXU and m.ntendon <= abi.MAXTENDON)


_cache = {}


def _compiled(key, text_fn):
    if key not in _cache:
        _cache[key] = mjcf.compile_xml_string(text_fn(), name_hint=key)
    return _cache[key]


# ------------------------------------------------------------------------------------------------
# the humanoids with a tail
# ------------------------------------------------------------------------------------------------
TAIL_LINKS = ("tail1", "tail2", "tail3")


def tail_xml(base="humanoid_mjx"):
    """The golden humanoid plus a three-link hinge chain of capsules, last child of the pelvis (so its dofs
    sit between the left leg's and the arms'): limited joints with damping, stiffness and armature, one motor
    per joint; the geoms collide with the floor and the left leg like the right leg's do. Keyframes get the
    tail at zero."""
    root = ET.fromstring(open(os.path.join(GOLDEN, base + ".xml")).read())
    pelvis = root.find(".//body[@name='pelvis']")
    parent = pelvis
    spec = [("-.09 0 .02", "0.9659 0 0.2588 0", "0 1 0", "-40 40", ".035"),
            ("-.2 0 0", "0.9914 0.1305 0 0", "0 0 1", "-50 50", ".03"),
            ("-.2 0 0", "0.9914 0 -0.1305 0", "0 1 0", "-60 30", ".025")]
    for name, (pos, quat, axis, rng, size) in zip(TAIL_LINKS, spec):
        b = ET.SubElement(parent, "body", name=name, pos=pos, quat=quat)
        ET.SubElement(b, "joint", name=name, pos=".01 0 0", axis=axis, range=rng, damping="1", stiffness="4",
                      armature=".02")
        ET.SubElement(b, "geom", name=name, fromto="-.02 0 0 -.18 0 0", size=size, contype="4", conaffinity="3")
        parent = b
    act = root.find("actuator")
    for name in TAIL_LINKS:
        ET.SubElement(act, "motor", name=name, gear="20", joint=name)
    # the tail's qpos address: compile once without keyframes
    keys = root.find("keyframe")
    root.remove(keys)
    adr = None
    m0 = mjcf.compile_xml_string(ET.tostring(root, encoding="unicode"))
    adr = int(m0.jnt_qposadr[m0.names["joint"].index("tail1")])
    for k in keys:
        q = k.get("qpos").split()
        k.set("qpos", " ".join(q[:adr] + ["0"] * len(TAIL_LINKS) + q[adr:]))
    root.append(keys)
    return ET.tostring(root, encoding="unicode")


TAIL_SENSORS = (
    '<jointpos name="jp_tail1" joint="tail1"/>', '<jointpos name="jp_knee" joint="knee_left"/>',
    '<framepos name="fp_tail3" objtype="xbody" objname="tail3"/>', '<framequat name="fq_tail3" objtype="xbody" objname="tail3"/>',
    '<framezaxis name="fz_site" objtype="site" objname="imu_tail"/>',
    '<touch name="touch_foot_right" site="site_foot_right"/>',
    '<jointvel name="jv_tail2" joint="tail2"/>', '<gyro name="gyro_tail" site="imu_tail"/>',
    '<velocimeter name="velo_tail" site="imu_tail"/>', '<framelinvel name="fl_tail3" objtype="xbody" objname="tail3"/>',
    '<frameangvel name="fa_site" objtype="site" objname="imu_tail"/>',
    '<touch name="touch_foot_left" site="site_foot_left"/>',
    '<accelerometer name="accel_tail" site="imu_tail"/>', '<jointlimitfrc name="jl_tail1" joint="tail1"/>',
    '<jointlimitfrc name="jl_tail3" joint="tail3"/>', '<jointlimitfrc name="jl_knee" joint="knee_left"/>',
    '<jointactuatorfrc name="ja_tail2" joint="tail2"/>', '<actuatorfrc name="af_tail3" actuator="tail3"/>',
    '<actuatorfrc name="af_knee" actuator="knee_left"/>')


def tail_sensors_xml():
    """`tail` with an IMU site on the last tail link (body 19, rotated, off the body origin) and a few sensors of
    each stage on the tail, the site and a leg joint, the two touch sensors among them."""
    root = ET.fromstring(tail_xml("humanoid_mjx"))
    t3 = root.find(".//body[@name='tail3']")
    ET.SubElement(t3, "site", name="imu_tail", pos="-.1 .01 .02", quat="0.7 0.1 -0.5 0.5", size="0.01")
    sens = root.find("sensor")
    for el in list(sens):
        sens.remove(el)
    for text in TAIL_SENSORS:
        sens.append(ET.fromstring(text))
    return ET.tostring(root, encoding="unicode")


def tail_sensors():
    return _compiled("tail_sensors", tail_sensors_xml)


def tail():
    return _compiled("tail", lambda: tail_xml("humanoid_mjx"))


def tail_euler():
    return _compiled("tail_euler", lambda: tail_xml("humanoid"))


# ------------------------------------------------------------------------------------------------
# one threshold each
# ------------------------------------------------------------------------------------------------
_HEAD = '<mujoco><option timestep="0.004" integrator="implicitfast" iterations="20" ls_iterations="20"/>'
_FLOOR = '<geom name="floor" type="plane" size="0 0 1" condim="3"/>'


def _f(*v):
    return " ".join(f"{x:.4f}" for x in v)


def nv_only_xml(n):
    """Two free roots over a plane; n limited, damped hinges, two per limb body (the last body one when n is
    odd), the bodies alternating between the roots as two chains; one motor per hinge.
    nv = 12 + n, njnt = 2 + n, nbody = ngeom = 3 + ceil(n / 2)."""
    nb = (n + 1) // 2
    chains = ["", ""]
    for i in reversed(range(nb)):
        r, k = i % 2, i // 2
        jn = ""
        for h in range(2 if 2 * i + 1 < n else 1):
            ax = ("0 1 0", "1 0 0.2", "0 1 1", "0 0 1")[(k + 2 * h) % 4]
            jn += (f'<joint name="h{2 * i + h}" axis="{ax}" pos="0.01 0 {_f(0.01 * h)}" range="-60 45" damping="0.3" '
                   f'armature="0.01" stiffness="{1 + k % 2}"/>')
        chains[r] = (f'<body name="l{i}" pos="{_f(0.16, 0.02 * (k % 2), -0.01)}">{jn}'
                     f'<geom type="capsule" fromto="0 0 0 0.14 0 {_f(0.02 * (1 - k % 2))}" size="0.03" condim="1"/>'
                     f'{chains[r]}</body>')
    roots = "".join(f'<body name="root{r}" pos="0 {_f(0.6 * r)} {_f(0.25 + 0.1 * r)}" quat="{q}"><freejoint/>'
                    f'<geom type="sphere" size="0.08"/>{chains[r]}</body>'
                    for r, q in enumerate(("1 0 0 0", "0.92388 0 0.38268 0")))
    motors = "".join(f'<motor name="h{i}" joint="h{i}" gear="{10 + 2 * (i % 3)}" ctrlrange="-1 1" ctrllimited="true"/>'
                     for i in range(n))
    return f"{_HEAD}<worldbody>{_FLOOR}{roots}</worldbody><actuator>{motors}</actuator></mujoco>"


def nbody_only_xml(n):
    """A free root and a chain of n more bodies over a plane; odd links carry a hinge, even links are welded to
    their parent (jointless, like the humanoid's head). nbody = 2 + n, nv = 6 + ceil(n / 2), ngeom = 2 + n."""
    chain = ""
    for i in reversed(range(n)):
        jnt = (f'<joint name="h{i}" axis="{("0 1 0", "0 0 1")[(i // 2) % 2]}" range="-35 35" damping="0.2" '
               f'armature="0.01"/>') if i % 2 == 0 else ""
        q = "1 0 0 0" if i % 3 else "0.98481 0.17365 0 0"
        chain = (f'<body name="b{i}" pos="0.09 0 0" quat="{q}">{jnt}'
                 f'<geom type="capsule" fromto="0 0 0 0.07 0 0" size="0.025" condim="1"/>{chain}</body>')
    motors = "".join(f'<motor name="h{i}" joint="h{i}" gear="5" ctrlrange="-1 1" ctrllimited="true"/>'
                     for i in range(0, n, 2))
    return (f'{_HEAD}<worldbody>{_FLOOR}<body name="root" pos="0 0 0.07"><freejoint/><geom type="sphere" size="0.05"/>'
            f'{chain}</body></worldbody><actuator>{motors}</actuator></mujoco>')


def njnt_only_xml(n):
    """n hinges, two per body (the last body one when n is odd), on a binary tree of bodies hanging from the
    world: no free joint, no floor. njnt = nv = n, nbody = 1 + ceil(n / 2)."""
    nb = (n + 1) // 2

    def body(i):
        kids = "".join(body(c) for c in (2 * i + 1, 2 * i + 2) if c < nb)
        j = f'<joint name="h{2 * i}" axis="0 1 0" pos="0 0 0.01" range="-70 70" damping="0.05" armature="0.005"/>'
        if 2 * i + 1 < n:
            j += f'<joint name="h{2 * i + 1}" axis="1 0 0.3" range="-50 60" damping="0.05" armature="0.005" stiffness="0.5"/>'
        y = 0.0 if i == 0 else (0.12 if i % 2 else -0.12) / (1 + (i - 1) // 2 // 2)
        return (f'<body name="b{i}" pos="0 {_f(y)} -0.2">{j}'
                f'<geom type="capsule" fromto="0 0 0 0 0 -0.17" size="0.02" contype="0" conaffinity="0"/>{kids}</body>')
    motors = "".join(f'<motor name="h{i}" joint="h{i}" gear="2"/>' for i in range(0, n, 3))
    return f"{_HEAD}<worldbody>{body(0)}</worldbody><actuator>{motors}</actuator></mujoco>"


def ngeom_only_xml(n):
    """One free body carrying n spheres (a 3-wide slab of them) over a plane. ngeom = 1 + n, nbody 2, nv 6."""
    g = "".join(f'<geom type="sphere" pos="{_f(0.1 * (i % 3), 0.1 * (i // 3), 0.015 * (i % 2))}" '
                f'size="{_f(0.05 + 0.004 * (i % 3))}" condim="{3 if i % 4 == 0 else 1}"/>' for i in range(n))
    return (f'{_HEAD}<worldbody>{_FLOOR}<body name="slab" pos="0 0 0.12" quat="0.99619 0.08716 0 0"><freejoint/>{g}'
            f'</body></worldbody></mujoco>')


def nv_only(n=16):
    return _compiled(f"nv_only{n}", lambda: nv_only_xml(n))


def nbody_only(n=16):
    return _compiled(f"nbody_only{n}", lambda: nbody_only_xml(n))


def njnt_only(n=23):
    return _compiled(f"njnt_only{n}", lambda: njnt_only_xml(n))


def ngeom_only(n=21):
    return _compiled(f"ngeom_only{n}", lambda: ngeom_only_xml(n))


# ------------------------------------------------------------------------------------------------
# at the capacities
# ------------------------------------------------------------------------------------------------
# per limb link: number of hinges (0 = welded to its parent). 5 limbs x 6 links = 30 bodies beside the root and
# the world: 7 welded, 20 with one hinge, 3 with two: 26 hinges, nv = 6 + 26 = 32
FULL_LIMBS = [(1, 2, 0, 1, 1, 0), (1, 1, 0, 2, 1, 1), (2, 0, 1, 1, 0, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1)]
FULL_COLLIDING = 23  # limb geoms (in body order) that also collide with each other: puts npair just under 256


def full_xml():
    """nv 32, nbody 32, ngeom 32, njnt 27: a free torso low over a plane with five limbs of six links radiating
    from it. Link frames are rotated about varying axes, capsules run obliquely in their body frames (inertia
    frames differ from body frames), hinges sit off the body origin, three bodies carry two hinges, seven are
    welded; two fixed tendons with limits, one motor per hinge."""
    rng = np.random.default_rng(20)
    limbs, hinges, nlink = "", [], 0
    axes = ("0 1 0", "0 0 1", "1 0 0.4", "0.3 1 0")
    for li, counts in enumerate(FULL_LIMBS):
        ang = 2 * np.pi * li / len(FULL_LIMBS)
        chain = ""
        for k in reversed(range(len(counts))):
            idx = nlink + k
            jn = ""
            for h in range(counts[k]):
                name = f"j{li}_{k}_{h}"
                jn += (f'<joint name="{name}" axis="{axes[(li + k + 2 * h) % 4]}" pos="{_f(0.01 * h, 0.005, 0.01)}" '
                       f'range="{-30 - 5 * k} {20 + 4 * li}" damping="{_f(0.4 + 0.1 * k)}" armature="0.01" '
                       f'stiffness="{_f(0.5 * (k % 3))}"/>')
            q = rng.normal(size=4) * 0.12 + [1, 0, 0, 0]
            q /= np.linalg.norm(q)
            if k == 0:  # the limb's direction in the torso frame
                q = mjcf.quat_mul(np.array([np.cos(ang / 2), 0, 0, np.sin(ang / 2)]), q)
            collide = 'contype="3" conaffinity="2"' if idx < FULL_COLLIDING else 'contype="1" conaffinity="0"'
            if k % 3 == 2:
                geom = f'<geom type="sphere" pos="0.05 0.01 0" size="0.04" condim="1" {collide}/>'
            else:
                geom = (f'<geom type="capsule" fromto="0.01 0 0 {_f(0.1, 0.02 * (k % 2) - 0.01, 0.015 * (li % 3) - 0.01)}" '
                        f'size="{_f(0.028 + 0.002 * (k % 3))}" condim="1" {collide}/>')
            pos = _f(0.12, 0, 0) if k else _f(0.1, 0, 0.0)
            chain = f'<body name="l{li}_{k}" pos="{pos}" quat="{_f(*q)}">{jn}{geom}{chain}</body>'
        for k in range(len(counts)):
            hinges += [f"j{li}_{k}_{h}" for h in range(counts[k])]
        nlink += len(counts)
        limbs += chain
    motors = "".join(f'<motor name="{j}" joint="{j}" gear="{4 + 2 * (i % 4)}" ctrlrange="-1 1" ctrllimited="true"/>'
                     for i, j in enumerate(hinges))
    tendons = ('<fixed name="t0" limited="true" range="-0.2 0.6"><joint joint="j0_0_0" coef=".5"/><joint joint="j0_1_1" '
               'coef="-.5"/></fixed><fixed name="t1" limited="true" range="-0.3 0.5"><joint joint="j4_0_0" coef=".6"/>'
               '<joint joint="j4_5_0" coef="-.4"/></fixed>')
    return (f'{_HEAD}<worldbody><geom name="floor" type="plane" size="0 0 1" condim="3" contype="1" conaffinity="1"/>'
            f'<body name="torso" pos="0 0 0.3"><freejoint/>'
            f'<geom type="sphere" size="0.09" contype="1" conaffinity="0"/>{limbs}</body></worldbody>'
            f'<tendon>{tendons}</tendon><actuator>{motors}</actuator></mujoco>')


def full():
    return _compiled("full", full_xml)


# name -> (builder, runs the generic kernels, the dims past the humanoid's)
MODELS = {
    "tail": (tail, True, {"nv", "nbody", "njnt", "ngeom"}),
    "tail_euler": (tail_euler, True, {"nv", "nbody", "njnt", "ngeom"}),
    "nv_only": (nv_only, True, {"nv"}),
    "nbody_only": (nbody_only, True, {"nbody"}),
    "njnt_only": (njnt_only, True, {"njnt"}),
    "ngeom_only": (ngeom_only, True, {"ngeom"}),
    "full": (full, True, {"nv", "nbody", "njnt", "ngeom"}),
    # one link fewer: exactly at a humanoid dim, still the humanoid kernels
    "nv_at": (lambda: nv_only(15), False, set()),
    "nbody_at": (lambda: nbody_only(15), False, set()),
    "njnt_at": (lambda: njnt_only(22), False, set()),
    "ngeom_at": (lambda: ngeom_only(19), False, set()),
}
GENERIC = [k for k, v in MODELS.items() if v[1]]
