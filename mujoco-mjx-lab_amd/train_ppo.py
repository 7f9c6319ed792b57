"""PPO on the MI355X-native humanoid env (reference train_ppo.py CLI: --test / --config).

Single GPU:   python mujoco-mjx-lab_amd/train_ppo.py [--config path/config.json] [--iterations N]
Multi-GPU:    python -m torch.distributed.run --nproc-per-node G --master-addr 127.0.0.1 \\
                  mujoco-mjx-lab_amd/train_ppo.py --num-envs 8192 ...   (envs split across ranks)
Results go to results/<timestamp>_ppo/{config.json,logs/metrics.jsonl,checkpoints/} as in the
reference (src/checkpoint_utils.py:13-100).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import mjx_amd  # noqa: E402
from mjx_amd import mjx  # noqa: E402
from mjx_amd.config import PPOConfig, reference_ppo_config  # noqa: E402
from mjx_amd.envs import HumanoidEnv, resolve_ids  # noqa: E402
from mjx_amd.ppo import PPOTrainer  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="reference-style config.json (env / ppo sections)")
    ap.add_argument("--test", action="store_true", help="tiny run (reference config_test.json spirit)")
    ap.add_argument("--iterations", type=int, default=None)
    ap.add_argument("--num-envs", type=int, default=None, help="total envs over all ranks")
    ap.add_argument("--model", default=None, help="humanoid_mjx | humanoid | path to .xml")
    ap.add_argument("--results-dir", default=None)
    ap.add_argument("--seed", type=int, default=None, help="override the config's seed")
    ap.add_argument("--jax-keys", action="store_true",
                    help="draw env resets from train_ppo.py's jax.random key chain (same reset stream as the reference)")
    ap.add_argument("--save-video", action="store_true",
                    help="per eval, write the policy rollout's qpos history (.npz) and its rendered video (.gif)")
    ap.add_argument("--push-force", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="random horizontal pushes on the training envs: force magnitude range in N (off by default)")
    ap.add_argument("--push-interval", type=int, nargs=2, metavar=("LO", "HI"), default=None,
                    help="env steps between pushes, drawn per env (default 100 200)")
    ap.add_argument("--push-duration", type=int, default=None, metavar="K", help="env steps a push lasts (default 5)")
    ap.add_argument("--push-body", default=None, metavar="NAME", help="pushed body (default: the env's pelvis body)")
    for name, what in (("mass", "body masses (inertias scale with them), one scale per body"),
                       ("friction", "sliding friction, one scale per geom (a pair takes the larger scaled value)"),
                       ("damping", "joint damping, one scale per dof"), ("armature", "armature, one scale per dof"),
                       ("gear", "actuator gear, one scale per actuator")):
        ap.add_argument(f"--rand-{name}", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                        help=f"domain randomisation of the training envs: {what}, uniform in [LO, HI] times the "
                             "model's value, drawn once at start (off by default)")
    ap.add_argument("--pd-control", type=float, nargs=2, metavar=("KP", "KV"), default=None,
                    help="joint-target actions: the motors become PD actuators (stiffness KP, damping KV) that hold "
                         "qpos0 + S * action within the motors' torque limits, in the training and evaluation envs "
                         "(off by default)")
    ap.add_argument("--action-scale", type=float, default=None, metavar="S",
                    help="radians of joint target per unit action with --pd-control (default 1)")
    ap.add_argument("--n-frames", type=int, default=1, metavar="K",
                    help="physics steps per env step, in the training and evaluation envs (the "
                         "action holds for all K, reward and observation come from the last; default 1)")
    a = ap.parse_args(argv)
    if not 1 <= a.n_frames <= 64:
        ap.error("--n-frames must be in 1..64")
    if a.action_scale is not None and a.pd_control is None:
        ap.error("--action-scale needs --pd-control KP KV")
    if a.push_force is None and (a.push_interval or a.push_duration is not None or a.push_body):
        ap.error("--push-interval / --push-duration / --push-body need --push-force LO HI")
    return a


def push_config(a, model, env_cfg):
    """PPOTrainer's `push` from the --push-* flags: None without --push-force (no attach, no new launches)."""
    if a.push_force is None:
        return None
    body = env_cfg.pelvis_body_id if a.push_body is None else model.name2id("body", a.push_body)
    if body < 1:
        raise SystemExit(f"--push-body: no body named {a.push_body!r}")
    return {"body": body, "interval": tuple(a.push_interval or (100, 200)),
            "duration": 5 if a.push_duration is None else a.push_duration, "force": tuple(a.push_force)}


def control_model(a, model):
    """The model the envs run: `model` itself without --pd-control (nothing new is built or launched), else its
    copy with PD actuators (mjx_amd.actuators.pd_actuators)."""
    if a.pd_control is None:
        return model
    from mjx_amd.actuators import pd_actuators
    return pd_actuators(model, a.pd_control[0], a.pd_control[1], 1.0 if a.action_scale is None else a.action_scale)


def randomize_config(a):
    """PPOTrainer's `randomize` from the --rand-* flags: None when none is given (no option set, no new kernel)."""
    r = {k: tuple(getattr(a, "rand_" + k)) for k in ("mass", "friction", "damping", "armature", "gear")
         if getattr(a, "rand_" + k) is not None}
    return r or None


def main():
    a = parse_args()
    cfg = PPOConfig.from_json(a.config) if a.config else reference_ppo_config()
    if a.test:
        cfg.num_envs, cfg.rollout_length, cfg.minibatch_size, cfg.total_iterations = 64, 16, 256, 3
        cfg.eval_interval = cfg.checkpoint_every = 2
    if a.num_envs:
        cfg.num_envs = a.num_envs
    if a.iterations:
        cfg.total_iterations = a.iterations
    if a.results_dir:
        cfg.results_dir = a.results_dir
    if a.seed is not None:
        cfg.seed = a.seed
    if a.save_video:
        cfg.save_video = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank, local = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    torch.cuda.set_device(local)
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    model = control_model(a, mjx_amd.load_model(a.model or os.path.splitext(os.path.basename(cfg.xml_path))[0]))
    sys_ = mjx.put_model(model)
    env_cfg = resolve_ids(model, cfg.env_config)
    env = HumanoidEnv(sys_, env_cfg, cfg.num_envs // world, device=local, seed=cfg.seed * 7919 + rank,
                      n_frames=a.n_frames)
    eval_env = HumanoidEnv(sys_, env_cfg, 32, device=local, seed=cfg.seed + 10000,
                           n_frames=a.n_frames) if rank == 0 else None
    out = None
    if rank == 0:
        out = os.path.join(cfg.results_dir, time.strftime("%Y%m%d_%H%M%S") + "_ppo")
    tr = PPOTrainer(cfg, env, eval_env, device=f"cuda:{local}", dist=dist, out_dir=out, jax_keys=a.jax_keys,
                    push=push_config(a, model, env_cfg), randomize=randomize_config(a))
    tr.train()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
