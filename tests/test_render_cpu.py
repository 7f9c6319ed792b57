"""Renderer, host side: the MJCF visual description, the fp64 reference renderer against closed forms
(the yardstick of tests/test_render_gpu.py, pinned independently of the kernel), the GIF writer and
the C ABI of the new entry points.

Marginal-pixel shares of the reference (render_ref.render_with_mask) on the scenes the GPU tests use,
computed here on the CPU; the cap is 1 % of an image (test_marginal_share_of_every_gpu_scene asserts it):
    humanoid 64x48, side_view, poses 0-3, shadows on / off   0.03 - 0.20 %
    humanoid 64x48, egocentric, poses 0-1                    0.07 %
    humanoid 50x37, side_view, poses 0-2 (ragged test)       0.00 - 0.43 %
    camera-modes scene 48x32, trk / com / fix                0.00 - 0.13 %
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mjx_amd
import render_ref
import render_scenes as rs
from mjx_amd import _lib, abi, mjcf, rendering
from mjx_amd._header import HEADER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def hum():
    return mjcf.compile_xml(os.path.join(GOLDEN, "humanoid_mjx.xml"))


def test_visual_description_of_humanoid_mjx(hum):
    v = hum.visual
    cams = {c["name"]: c for c in v["cameras"]}
    assert list(cams) == ["track", "back_view", "side_view", "egocentric"]
    sv = cams["side_view"]
    assert sv["body"] == hum.name2id("body", "torso") and sv["mode"] == "trackcom" and sv["fovy"] == 45.0
    # xyaxes="1 0 0 0 0 1": x right = world x, y up = world z, so the camera looks along +y
    assert np.allclose(np.array(sv["mat"]).reshape(3, 3), [[1, 0, 0], [0, 0, -1], [0, 1, 0]])
    kin = mjcf._fk_and_mass(hum, hum.qpos0)
    t = sv["body"]
    assert np.allclose(np.array(sv["pos0_trackcom"]) + kin["subtree_com"][t], kin["xpos"][t] + [0, -3, -0.3])
    assert np.allclose(np.array(sv["pos0_track"]), [0, -3, -0.3])
    ego = cams["egocentric"]
    assert ego["mode"] == "fixed" and ego["fovy"] == 80.0 and ego["body"] == hum.name2id("body", "head")
    R = np.array(ego["mat"]).reshape(3, 3)
    assert np.allclose(R.T @ R, np.eye(3)) and np.allclose(R[:, 0], [0, -1, 0]) and np.linalg.det(R) > 0
    rgba = np.array(v["geom_rgba"])
    assert np.allclose(rgba[hum.name2id("geom", "torso")], [0.8, 0.6, 0.4, 1])
    assert np.allclose(rgba[1:], [0.8, 0.6, 0.4, 1])  # every body geom takes material "body" from its class
    ck = v["checker"]
    assert ck["geom"] == hum.name2id("geom", "floor") and ck["rgb1"] == [0.1, 0.2, 0.3] and ck["rgb2"] == [0.2, 0.3, 0.4]
    assert ck["cell"] == [0.5, 0.5]  # texuniform, texrepeat 1: the 2 x 2 checker image spans 1 m
    assert v["sky"] == {"rgb1": [0.3, 0.5, 0.7], "rgb2": [0.0, 0.0, 0.0]} and v["zfar"] == 30.0
    L = v["light"]  # the first light: "spotlight", aimed at the torso's subtree com at qpos0
    assert L["pos"] == [0.0, -6.0, 4.0] and L["diffuse"] == [0.8, 0.8, 0.8] and not L["directional"]
    aim = kin["subtree_com"][t] - np.array(L["pos"])
    assert np.allclose(L["dir"], aim / np.linalg.norm(aim))


def test_both_humanoids_compile_with_unchanged_arrays_and_shipped_visuals():
    for name in mjx_amd.BUILTIN_MODELS:
        fresh = mjcf.compile_xml(os.path.join(GOLDEN, name + ".xml"))
        asset = mjx_amd.load_model(name)
        assert set(asset.arrays) == set(fresh.arrays)
        for k, a in fresh.arrays.items():
            np.testing.assert_array_equal(asset.arrays[k], a, err_msg=k)
        assert "visual" not in fresh.to_json_dict()
        assert asset.visual == fresh.visual  # assets/<name>_visual.json is what a fresh compile gives
        assert abi.visual_desc(asset).ncam == 4


def test_geom_rgba_precedence_and_camera_errors():
    m = mjcf.compile_xml_string("""<mujoco><asset><material name="m" rgba="0 1 0 1"/></asset>
      <default><default class="c"><geom rgba="0 0 1 1"/></default></default>
      <worldbody><geom type="plane" size="1 1 .1"/>
        <camera name="ok" pos="0 0 3" quat="1 0 0 0"/><camera name="tb" mode="targetbody" target="b"/>
        <camera name="eu" euler="0 0 90"/>
        <body name="b" pos="0 0 1"><freejoint/><geom size=".1" rgba="1 0 0 1" material="m" class="c"/>
          <geom size=".1" material="m" class="c"/><geom size=".1" class="c"/></body></worldbody></mujoco>""")
    assert m.visual["geom_rgba"] == [[0.5, 0.5, 0.5, 1.0], [1, 0, 0, 1], [0, 1, 0, 1], [0, 0, 1, 1]]
    assert m.visual["checker"] is None and m.visual["sky"]["rgb1"] == m.visual["sky"]["rgb2"]
    assert mjcf.camera_id(m, "ok") == 0 and mjcf.camera_id(m, 0) == 0
    with pytest.raises(mjcf.MJCFError, match="'tb'.*targetbody"):
        mjcf.camera_id(m, "tb")
    with pytest.raises(mjcf.MJCFError, match="'eu'.*euler"):
        mjcf.camera_id(m, 2)
    with pytest.raises(mjcf.MJCFError, match="nope"):
        mjcf.camera_id(m, "nope")
    assert [abi.visual_desc(m).cam_mode[i] for i in range(3)] == [abi.CAM_MODE["fixed"], -1, -1]


def test_reference_sphere_against_closed_forms():
    """33 x 25: the centre pixel's ray is the camera axis, so its depth is d - r exactly."""
    m = mjcf.compile_xml_string(rs.SPHERE_XML)
    W, H = 33, 25
    rgb, dep, seg, _ = render_ref.render(m, m.qpos0, "cam", W, H)
    assert seg[12, 16] == 1 and dep[12, 16] == pytest.approx(rs.KAT_D - rs.SPHERE_R, rel=1e-12)
    assert seg[13, 17] == 1 and dep[13, 17] == pytest.approx(rs.sphere_depth(rs.pixel_dir(17, 13, W, H), (0, 0, 1), rs.SPHERE_R), rel=1e-12)
    assert seg[24, 3] == 0 and dep[24, 3] == pytest.approx(rs.floor_depth(rs.pixel_dir(3, 24, W, H)), rel=1e-12)
    assert seg[0, 16] == -1 and np.isinf(dep[0, 16])
    # the sphere's outline: a pixel is on the sphere iff its ray passes within r of the centre
    for j in range(H):
        for i in range(W):
            d = rs.pixel_dir(i, j, W, H)
            c = np.array([0, rs.KAT_D, 0.0])
            assert (seg[j, i] == 1) == (np.linalg.norm(c - np.dot(c, d) * d) < rs.SPHERE_R)
    # sky: no skybox in this scene, a constant background; the sphere's lit side is its own colour scaled
    assert (rgb[0, 16] == 0).all() and rgb[12, 16, 0] > rgb[12, 16, 1] == rgb[12, 16, 2]


def test_reference_capsule_against_closed_forms():
    m = mjcf.compile_xml_string(rs.CAPSULE_XML)
    W, H = 33, 25
    _, dep, seg, _ = render_ref.render(m, m.qpos0, "cam", W, H)
    assert seg[12, 16] == 1 and dep[12, 16] == pytest.approx(rs.KAT_D - rs.CAPSULE_R, rel=1e-12)  # cylinder side
    d = rs.pixel_dir(18, 13, W, H)
    assert seg[13, 18] == 1 and dep[13, 18] == pytest.approx(rs.xcylinder_depth(d), rel=1e-12)
    # towards the tip: move the rays so that pixel (16, 12) looks at the cap centre (0.6, 0, 1). That ray is
    # oblique and enters through the cylinder side just before the cap; a ray past x = 0.6 + r misses
    th = np.tan(0.5 * np.deg2rad(rs.KAT_FOVY))
    dx = (rs.CAPSULE_H / rs.KAT_D) / (th * W / H) * W / 2
    _, dep2, seg2, _ = render_ref.render(m, m.qpos0, "cam", W, H, dx=dx)
    d2 = np.array([rs.CAPSULE_H, rs.KAT_D, 0.0]) / np.hypot(rs.KAT_D, rs.CAPSULE_H)
    assert seg2[12, 16] == 1 and dep2[12, 16] == pytest.approx(rs.xcylinder_depth(d2), rel=1e-12)
    assert dep2[12, 16] * d2[0] < rs.CAPSULE_H  # on the side indeed
    dx_out = ((rs.CAPSULE_H + 1.2 * rs.CAPSULE_R) / rs.KAT_D) / (th * W / H) * W / 2
    assert render_ref.render(m, m.qpos0, "cam", W, H, dx=dx_out)[2][12, 16] != 1
    # the hemisphere: a ray that meets the cap beyond the cylinder's end, the sphere closed form about the cap centre
    dd = rs.pixel_dir(16, 12, W, H)  # unshifted direction of the centre pixel = (0, 1, 0)
    u_tip = (rs.CAPSULE_H + 0.5 * rs.CAPSULE_R) / rs.KAT_D
    d3 = np.array([u_tip, 1.0, 0.0]) / np.hypot(u_tip, 1.0)
    dx3 = u_tip / (th * W / H) * W / 2
    _, dep3, seg3, _ = render_ref.render(m, m.qpos0, "cam", W, H, dx=dx3)
    assert seg3[12, 16] == 1 and dep3[12, 16] == pytest.approx(rs.sphere_depth(d3, (rs.CAPSULE_H, 0, 1), rs.CAPSULE_R), rel=1e-12)
    assert dd == pytest.approx([0, 1, 0])


def _gpu_scenes():
    hum = rs.humanoid()
    poses = rs.humanoid_poses(hum)
    for k, q in enumerate(poses):
        for sh in (True, False):
            yield f"hum side_view pose{k} shadows={sh}", hum, q, "side_view", 64, 48, sh
    for k in range(2):
        yield f"hum egocentric pose{k}", hum, poses[k], "egocentric", 64, 48, True
    for k in range(3):
        yield f"hum ragged pose{k}", hum, poses[k], "side_view", 50, 37, True
    mm = mjcf.compile_xml_string(rs.MODES_XML)
    q = mm.qpos0.copy()
    q[7] = 0.7
    for cam in ("trk", "com", "fix"):
        yield f"modes {cam}", mm, q, cam, 48, 32, True


def test_marginal_share_of_every_gpu_scene():
    """The condition of the GPU comparisons: at most 1 % of any test image is marginal."""
    for name, m, q, cam, W, H, sh in _gpu_scenes():
        marg = render_ref.render_with_mask(m, q, cam, W, H, sh)[3]
        print(f"{name}: {100 * marg.mean():.2f} % marginal")
        assert marg.mean() <= 0.01, name


def test_save_video_gif_round_trip(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(3)
    palette = rng.integers(0, 256, (200, 3), dtype=np.uint8)  # <= 256 colours over all five frames
    frames = palette[rng.integers(0, 200, (5, 24, 32))]
    path = rendering.save_video(str(tmp_path / "v" / "clip.gif"), frames, fps=25)
    assert path.endswith("clip.gif")
    with Image.open(path) as im:
        assert im.n_frames == 5 and im.size == (32, 24) and im.info["duration"] == 40
        for i in range(5):
            im.seek(i)
            np.testing.assert_array_equal(np.asarray(im.convert("RGB")), frames[i])


def test_save_video_without_pil_writes_npy(tmp_path, monkeypatch, capsys):
    import builtins
    real = builtins.__import__

    def no_pil(name, *a, **k):
        if name == "PIL" or name.startswith("PIL."):
            raise ImportError(name)
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_pil)
    frames = np.zeros((2, 4, 6, 3), np.uint8)
    path = rendering.save_video(str(tmp_path / "clip.gif"), frames, fps=30)
    assert path.endswith("clip.npy") and np.array_equal(np.load(path), frames)
    assert "PIL is not installed" in capsys.readouterr().err


def test_frame_stride_is_the_references():
    assert rendering.frame_stride(0.005, 60) == 3 and rendering.frame_stride(0.02, 60) == 1


def test_render_entry_points_in_derived_binding():
    names = ("mjl_renderer_create", "mjl_renderer_destroy", "mjl_render_qpos")
    assert all(n in _lib.EXPORTS for n in names)
    L = _lib.lib()
    vp, i32 = C.c_void_p, C.c_int
    assert L.mjl_renderer_create.argtypes == [vp, C.POINTER(abi.VisualDesc), i32, i32, C.POINTER(vp)]
    assert L.mjl_renderer_destroy.argtypes == [vp] and L.mjl_renderer_destroy.restype is None
    assert L.mjl_render_qpos.argtypes == [vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    assert HEADER.enums["MJL_CAM_TRACKCOM"] == 2 and HEADER.enums["MJL_RENDER_SHADOWS"] == 1 and HEADER.defines["MJL_MAXCAM"] == 8
    # argument errors are reported before any device call
    assert L.mjl_renderer_create(None, None, 1, 0, C.byref(vp())) == 1
    assert L.mjl_render_qpos(None, None, 1, 0, 8, 8, 0, None, None, None, None) == 1


def test_visual_desc_layout_matches_c_compiler(tmp_path):
    """sizeof and the last field's offset of mjlVisualDesc from a compiled probe; mjlModelDesc and
    mjlEnvConfig keep the sizes the binding derives (the oracle build checks those against its own compile)."""
    src = tmp_path / "probe.cpp"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mjx355.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mjlVisualDesc), offsetof(mjlVisualDesc, cam_mat0),'
                   ' sizeof(mjlModelDesc), sizeof(mjlEnvConfig)); return 0; }\n')
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert abi.VisualDesc._fields_[-1][0] == "cam_mat0"
    assert got == [C.sizeof(abi.VisualDesc), abi.VisualDesc.cam_mat0.offset, C.sizeof(abi.ModelDesc), C.sizeof(abi.EnvConfigC)]
