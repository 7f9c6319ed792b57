"""The ray-cast renderer on the GPU (mjl_render_qpos) against closed forms and the fp64 reference
(tests/render_ref.py), on the reference's non-marginal pixels (its mask: at most 1 % of every image here,
figures in tests/test_render_cpu.py's header, asserted there and again here).

Tolerances
  closed-form depth  1e-5 relative. A depth is ~40 fp32 operations on values of magnitude <= 3.3 m (ray
                     set-up and normalisation, offset to the centre, closest approach, root): each
                     rounds at 2^-24 = 6e-8 relative to its operands, the final subtraction b - th (3 m
                     minus <= 0.25 m) does not amplify, so the error is a few 1e-7 relative; 1e-5 leaves
                     a factor ~30 for sqrt / division approximations (the library builds with -fapprox-func).
  colour             1 LSB per channel: the quantisation step, one rounding flip is inherent.
  depth vs fp64      DEPTH_TOL = 8 x the largest relative depth error measured on these scenes
                     (profiles/r11/render_depth_error.txt), and at most 1e-3, the mask's own depth threshold.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import render_ref
import render_scenes as rs
from mjx_amd import _lib, abi, mjcf, mjx
from mjx_amd.render import Renderer

pytestmark = pytest.mark.gpu

DEPTH_TOL = 8 * 2.040e-06  # = 1.632e-05; 2.040e-06 is the measured maximum (side_view, pose 3)
KAT_TOL = 1e-5


@functools.lru_cache(maxsize=None)
def _hum():
    m = rs.humanoid()
    return m, mjx.put_model(m), [np.asarray(q) for q in rs.humanoid_poses(m)]


@functools.lru_cache(maxsize=None)
def _hum_renderer():
    return Renderer(_hum()[1], max_frames=8)


@functools.lru_cache(maxsize=None)
def _ref(pose, camera, W, H, shadows):
    m, _, poses = _hum()
    return render_ref.render_with_mask(m, poses[pose], camera, W, H, shadows)


def _compare(got, ref, what):
    """got: Frames of one image (tensors [H, W, .]); ref: (rgb, depth, seg, marginal mask)."""
    rgb, dep, seg, marg = ref
    assert marg.mean() <= 0.01, f"{what}: {100 * marg.mean():.2f} % of the reference image is marginal"
    ok = ~marg
    g_seg, g_dep, g_rgb = got.seg.cpu().numpy(), got.depth.cpu().numpy(), got.rgb.cpu().numpy()
    assert np.array_equal(g_seg[ok], seg[ok]), f"{what}: {(g_seg[ok] != seg[ok]).sum()} segmentation ids differ"
    d_rgb = np.abs(g_rgb.astype(int) - rgb.astype(int))[ok].max()
    hit = ok & (seg >= 0)
    assert np.array_equal(np.isinf(g_dep[ok]), np.isinf(dep[ok]))
    rel = (np.abs(g_dep[hit] - dep[hit]) / dep[hit]).max() if hit.any() else 0.0
    print(f"{what}: max colour diff {d_rgb} LSB, max relative depth error {rel:.3e}")
    assert d_rgb <= 1, what
    assert rel <= DEPTH_TOL, what
    return rel


def _one(frames, i):
    return type(frames)(*(None if t is None else t[i] for t in frames))


@pytest.mark.parametrize("xml", ["sphere", "capsule"])
def test_closed_form_kats(xml):
    m = mjcf.compile_xml_string(rs.SPHERE_XML if xml == "sphere" else rs.CAPSULE_XML)
    W, H = 48, 32
    out = Renderer(mjx.put_model(m), 1).render(torch.tensor(m.qpos0[None], dtype=torch.float32), "cam", W, H,
                                               depth=True, seg=True)
    dep, seg = out.depth[0].cpu().numpy(), out.seg[0].cpu().numpy()
    checks = []
    if xml == "sphere":
        for i, j in ((23, 15), (24, 16), (22, 17), (25, 14)):  # around the centre
            checks.append((i, j, 1, rs.sphere_depth(rs.pixel_dir(i, j, W, H), (0, 0, 1), rs.SPHERE_R)))
    else:
        for i, j in ((23, 15), (24, 16), (17, 15), (31, 16)):  # the cylinder side, along its length
            checks.append((i, j, 1, rs.xcylinder_depth(rs.pixel_dir(i, j, W, H))))
        # the hemispheres: pixels whose rays pass the cylinder's ends (|x| > 0.6 at the surface)
        th = math.tan(0.5 * math.radians(rs.KAT_FOVY))
        i_tip = int(((rs.CAPSULE_H + 0.6 * rs.CAPSULE_R) / rs.KAT_D / (th * W / H) + 1) * W / 2)
        for i, sx in ((i_tip, 1.0), (W - 1 - i_tip, -1.0)):
            for j in (15, 16):
                d = rs.pixel_dir(i, j, W, H)
                t = rs.sphere_depth(d, (sx * rs.CAPSULE_H, 0, 1), rs.CAPSULE_R)
                assert abs(t * d[0]) > rs.CAPSULE_H  # the chosen pixel does look at a cap
                checks.append((i, j, 1, t))
    for i, j in ((3, 31), (24, 30), (44, 28)):
        checks.append((i, j, 0, rs.floor_depth(rs.pixel_dir(i, j, W, H))))
    for i, j, g, want in checks:
        assert seg[j, i] == g, (i, j)
        print(f"{xml} pixel ({i}, {j}): depth {dep[j, i]:.7f}, closed form {want:.7f}, rel {abs(dep[j, i] - want) / want:.2e}")
        assert abs(dep[j, i] - want) <= KAT_TOL * want, (i, j)
    assert (seg[0] == -1).all() and np.isinf(dep[0]).all()  # the top row is sky


@pytest.mark.parametrize("shadows", [True, False])
def test_humanoid_side_view_against_reference(shadows):
    _, _, poses = _hum()
    q = torch.tensor(np.stack(poses), dtype=torch.float32)
    out = _hum_renderer().render(q, "side_view", 64, 48, shadows=shadows, depth=True, seg=True)
    for k in range(4):
        _compare(_one(out, k), _ref(k, "side_view", 64, 48, shadows), f"side_view pose {k} shadows={shadows}")


def test_humanoid_egocentric_against_reference():
    _, _, poses = _hum()
    q = torch.tensor(np.stack(poses[:2]), dtype=torch.float32)
    out = _hum_renderer().render(q, "egocentric", 64, 48, depth=True, seg=True)
    for k in range(2):
        _compare(_one(out, k), _ref(k, "egocentric", 64, 48, True), f"egocentric pose {k}")


def test_ragged_size_keeps_guard_bands():
    """3 frames at 50 x 37 (neither a multiple of the 16 x 16 tile) into buffers with 64 guard elements on both sides."""
    m, sys_, poses = _hum()
    n, W, H, G = 3, 50, 37, 64
    dev = torch.device("cuda")
    bufs = {"rgb": torch.full((G + n * H * W * 3 + G,), 0xA5, dtype=torch.uint8, device=dev),
            "depth": torch.full((G + n * H * W + G,), -777.0, dtype=torch.float32, device=dev),
            "seg": torch.full((G + n * H * W + G,), -12345, dtype=torch.int32, device=dev)}
    canary = {k: v[:G].clone() for k, v in bufs.items()}
    inner = {k: v[G:v.numel() - G] for k, v in bufs.items()}
    q = torch.tensor(np.stack(poses[:n]), dtype=torch.float32, device=dev)
    r = _hum_renderer()
    _lib.check(_lib.lib().mjl_render_qpos(r.handle, C.c_void_p(q.data_ptr()), n, mjcf.camera_id(m, "side_view"), W, H,
                                          abi.RENDER_SHADOWS, C.c_void_p(inner["rgb"].data_ptr()),
                                          C.c_void_p(inner["depth"].data_ptr()), C.c_void_p(inner["seg"].data_ptr()),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert torch.equal(v[:G], canary[k]) and torch.equal(v[-G:], canary[k]), f"{k}: guard band overwritten"
    from mjx_amd.render import Frames
    out = Frames(inner["rgb"].view(n, H, W, 3), inner["depth"].view(n, H, W), inner["seg"].view(n, H, W))
    assert not (out.seg == -12345).any() and not (out.depth == -777.0).any()  # every pixel was written
    for k in range(n):
        _compare(_one(out, k), _ref(k, "side_view", W, H, True), f"ragged pose {k}")


def test_batch_invariance_and_single_output():
    _, _, poses = _hum()
    q = torch.tensor(np.stack([poses[k % 4] for k in range(5)]), dtype=torch.float32, device="cuda")
    q[4, 0] += 0.37
    r = _hum_renderer()
    full = r.render(q, "side_view", 40, 24, depth=True, seg=True)
    for i in range(5):
        one = r.render(q[i:i + 1], "side_view", 40, 24, depth=True, seg=True)
        for a, b in zip(one, full):
            assert torch.equal(a[0], b[i]), i
    only = r.render(q, "side_view", 40, 24, rgb=False, depth=True)
    assert only.rgb is None and only.seg is None and torch.equal(only.depth, full.depth)


def test_camera_modes():
    """trackcom and track cameras follow a root translation; a fixed camera on a rotated body matches the reference."""
    m, _, poses = _hum()
    r = _hum_renderer()
    q0 = torch.tensor(poses[1][None], dtype=torch.float32)
    q1 = q0.clone()
    q1[0, :3] += torch.tensor([5.0, 3.0, 0.0])  # whole checker periods: the floor pattern repeats too

    def same(r_, qa, qb, cam, W, H):
        a = r_.render(qa, cam, W, H, depth=True, seg=True)
        b = r_.render(qb, cam, W, H, depth=True, seg=True)
        assert torch.equal(a.seg, b.seg), cam
        body = (a.seg > 0).cpu().numpy()[0]
        da, db = a.depth.cpu().numpy()[0][body], b.depth.cpu().numpy()[0][body]
        assert body.any() and (np.abs(da - db) <= DEPTH_TOL * da).all(), cam
    same(r, q0, q1, "side_view", 64, 48)
    mm = mjcf.compile_xml_string(rs.MODES_XML)
    rm = Renderer(mjx.put_model(mm), 2)
    qa = mm.qpos0.copy()
    qa[7] = 0.7  # the arm's hinge: the `fix` camera turns with it
    qb = qa.copy()
    qb[:3] += [5.0, 3.0, 0.0]
    ta, tb = (torch.tensor(x[None], dtype=torch.float32) for x in (qa, qb))
    same(rm, ta, tb, "trk", 48, 32)
    same(rm, ta, tb, "com", 48, 32)
    for cam in ("fix", "trk", "com"):
        out = rm.render(tb, cam, 48, 32, depth=True, seg=True)
        _compare(_one(out, 0), render_ref.render_with_mask(mm, qb, cam, 48, 32, True), f"modes scene, camera {cam}")


def test_errors_set_last_error_and_launch_nothing():
    m, sys_, poses = _hum()
    L = _lib.lib()
    r = _hum_renderer()  # max_frames 8
    dev = torch.device("cuda")
    q = torch.tensor(np.stack([poses[0]] * 9), dtype=torch.float32, device=dev)
    seg = torch.full((9, 8, 8), -5, dtype=torch.int32, device=dev)
    qp, sp, st = C.c_void_p(q.data_ptr()), C.c_void_p(seg.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ARG, UNSUP = 1, 2
    for args, word in (((qp, 9, 2, 8, 8, 0, None, None, sp, st), "frames"),
                       ((qp, 1, 2, 0, 8, 0, None, None, sp, st), "size"),
                       ((qp, 1, 4, 8, 8, 0, None, None, sp, st), "camera"),
                       ((qp, 1, -1, 8, 8, 0, None, None, sp, st), "camera"),
                       ((qp, 1, 2, 8, 8, 0, None, None, None, st), "no output")):
        assert L.mjl_render_qpos(r.handle, *args) == ARG
        assert word in L.mjl_last_error().decode()
    torch.cuda.synchronize()
    assert (seg == -5).all()  # nothing was launched
    with pytest.raises(_lib.MjlError, match="MJL_ERR_ARG"):
        r.render(q, "side_view", 8, 8)
    bad = abi.model_desc(m)
    bad.geom_type[3] = 6  # a box
    h, hr = C.c_void_p(), C.c_void_p()
    assert L.mjl_model_create(C.byref(bad), C.byref(h)) == 0
    vis = abi.visual_desc(m)
    assert L.mjl_renderer_create(h, C.byref(vis), 4, 0, C.byref(hr)) == UNSUP and not hr.value
    assert "geom 3" in L.mjl_last_error().decode()
    L.mjl_model_destroy(h)


def test_env_render_and_trainer_video(tmp_path):
    from PIL import Image

    from mjx_amd import rendering
    from mjx_amd.config import reference_ppo_config
    from mjx_amd.envs import HumanoidEnv, resolve_ids
    from mjx_amd.ppo import PPOTrainer
    m, sys_, _ = _hum()
    cfg = reference_ppo_config()
    env_cfg = resolve_ids(m, cfg.env_config)
    env = HumanoidEnv(sys_, env_cfg, 8, seed=3)
    env.reset()
    env.step(torch.zeros((8, env.act_dim), device="cuda"))
    got = env.render(seg=True, width=32, height=24)
    want = Renderer(sys_, 8).render(env.data.get("qpos"), "side_view", 32, 24, seg=True)
    assert got.rgb.shape == (8, 24, 32, 3) and got.seg.shape == (8, 24, 32) and got.depth is None
    assert torch.equal(got.rgb, want.rgb) and torch.equal(got.seg, want.seg)
    assert (got.seg > 0).any()
    # the trainer hook: a 1-env trainer writes the .gif beside the unchanged .npz
    cfg.num_envs, cfg.rollout_length, cfg.minibatch_size, cfg.total_iterations = 1, 4, 4, 1
    cfg.save_video, cfg.render_duration, cfg.render_width, cfg.render_height = True, 0.1, 32, 24
    tr = PPOTrainer(cfg, HumanoidEnv(sys_, env_cfg, 1, seed=5), HumanoidEnv(sys_, env_cfg, 1, seed=6), device="cuda:0",
                    out_dir=str(tmp_path))
    npz = tr.dump_qpos_history(0)
    hist = rendering.load_qpos_history(npz)
    steps, stride = hist["qpos"].shape[0], int(hist["stride"])
    assert steps == int(0.1 / float(m.timestep)) and stride == rendering.frame_stride(float(m.timestep), cfg.render_fps)
    assert sorted(hist) == sorted(["qpos", "act", "dt", "fps", "stride", "duration", "model", "camera_name"])
    with Image.open(os.path.join(str(tmp_path), "videos", "iter_000001.gif")) as im:
        assert im.n_frames == math.ceil(steps / stride) and im.size == (32, 24)
