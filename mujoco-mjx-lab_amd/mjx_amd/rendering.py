"""Policy-rollout videos (reference src/rendering.py:57-195): the qpos history, its frames, the file.

The reference scans `duration / dt` env steps of a deterministic policy on one env, resetting to the
rollout's own initial state whenever the env is done, collects `qpos` after every step and renders
the history with mujoco.Renderer (every `1 / (fps dt)`-th frame). Here `rollout_qpos_history` is that
scan, `render_qpos_history` renders the strided history with the ray-cast renderer (render.py; no
mujoco, no GL) and `save_video` writes the frames as an animated GIF. The history is also written as
an `.npz`, which any MuJoCo install renders offline with the reference's own loop
(`mj_data.qpos[:] = qpos[i]; mj_forward; renderer.render()`):

    qpos [T, nq]   post-step (post-reset-merge) qpos, as the reference's scan returns it
    act  [T, nu]   the clipped actions that produced it (replayable through the env)
    dt, fps, stride, duration, model, camera_name
"""
from __future__ import annotations

import os
from typing import Callable, Optional

import numpy as np
import torch


@torch.no_grad()
def rollout_qpos_history(env, policy_fn: Callable[[torch.Tensor], torch.Tensor], duration: float,
                         reset_keys: Optional[torch.Tensor] = None):
    """render_policy_rollout's scan (src/rendering.py:102-180) on a HumanoidEnv with B envs
    (B = 1 in the reference): action = clip(policy_fn(obs), -1, 1); step without the auto-reset;
    done envs go back to the rollout's initial state and obs. Returns (qpos [T, B, nq], act [T, B, nu])
    as numpy arrays. `reset_keys` [B, 2]: draw the initial state from jax.random keys
    (single_reset(key), src/rendering.py:91-93)."""
    dt = float(env.sys.m.timestep)
    steps = int(duration / dt)
    if reset_keys is not None:
        env.set_reset_keys(reset_keys.to(torch.int32).contiguous())
    obs0 = env.reset().clone()
    if reset_keys is not None:
        env.set_reset_keys(None)
    st0 = env.get_state().clone()
    B = env.num_envs
    qpos = torch.empty((steps, B, env.sys.nq), device=obs0.device)
    act = torch.empty((steps, B, env.act_dim), device=obs0.device)
    obs = obs0
    for t in range(steps):
        a = torch.clamp(policy_fn(obs), -1.0, 1.0)
        act[t] = a
        o, _, te, tr = env.step(a, auto_reset=False)
        done = torch.maximum(te, tr) > 0.5
        env.set_state(torch.where(done[:, None], st0, env.get_state()))
        obs = torch.where(done[:, None], obs0, o).clone()
        qpos[t] = env.data.get("qpos")
    return qpos.cpu().numpy(), act.cpu().numpy()


def save_qpos_history(path: str, qpos: np.ndarray, act: np.ndarray, dt: float, fps: int = 60,
                      model: str = "", camera_name: str = "side_view") -> str:
    """Write the history (one env: [T, nq]) next to where the reference writes its video
    (training_dir/videos/<prefix>_<step+1:06d>.npz instead of .mp4, training_utils.py:191-195)."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    stride = frame_stride(dt, fps)
    np.savez(path, qpos=qpos, act=act, dt=dt, fps=fps, stride=stride, duration=qpos.shape[0] * dt,
             model=model, camera_name=camera_name)
    return path


def load_qpos_history(path: str) -> dict:
    """Read a dump back (plain arrays, no pickle)."""
    with np.load(path, allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def frame_stride(dt: float, fps: int) -> int:
    """Every how many steps the reference takes a frame (src/rendering.py:184)."""
    return max(1, int(1.0 / (fps * dt)))


@torch.no_grad()
def render_qpos_history(renderer, qpos, stride: int = 1, camera="side_view", width: int = 640, height: int = 480,
                        shadows: bool = True) -> np.ndarray:
    """Frames uint8 [ceil(T / stride), H, W, 3] of a qpos history [T, nq] (numpy or torch), every
    `stride`-th step as src/rendering.py:186 takes them, rendered in chunks of the renderer's max_frames."""
    q = torch.as_tensor(np.asarray(qpos) if not torch.is_tensor(qpos) else qpos)[::stride]
    out = np.empty((q.shape[0], height, width, 3), np.uint8)
    for i in range(0, q.shape[0], renderer.max_frames):
        chunk = q[i:i + renderer.max_frames]
        out[i:i + chunk.shape[0]] = renderer.render(chunk, camera, width, height, shadows).rgb.cpu().numpy()
    return out


def save_video(path: str, frames: np.ndarray, fps: int = 60) -> str:
    """Write frames uint8 [T, H, W, 3] as an animated GIF at `path` (frame time rounded to GIF's 10 ms
    units; each frame quantised to its own palette of up to 256 colours) and return the path written. Without
    PIL the frames go to `<path minus extension>.npy` instead, and a line on stderr says so."""
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    try:
        from PIL import Image
    except ImportError:
        import sys
        alt = os.path.splitext(path)[0] + ".npy"
        np.save(alt, frames)
        print(f"save_video: PIL is not installed; wrote the raw frames to {alt} instead of {path}", file=sys.stderr)
        return alt
    # one palette per frame: the frame's own colours where they fit (exact), else PIL's adaptive quantiser
    imgs = []
    for f in frames:
        key = (f[..., 0].astype(np.uint32) << 16) | (f[..., 1].astype(np.uint32) << 8) | f[..., 2]
        uniq, inv = np.unique(key, return_inverse=True)
        if uniq.size <= 256:
            im = Image.frombytes("P", (f.shape[1], f.shape[0]), inv.astype(np.uint8).tobytes())
            im.putpalette(np.stack([uniq >> 16, (uniq >> 8) & 255, uniq & 255], axis=1).astype(np.uint8).tobytes())
        else:
            im = Image.fromarray(f).quantize(colors=256, dither=Image.Dither.NONE)
        imgs.append(im)
    imgs[0].save(path, save_all=True, append_images=imgs[1:], duration=max(10, int(round(1000.0 / fps / 10.0)) * 10),
                 loop=0, disposal=1, optimize=False)
    return path
