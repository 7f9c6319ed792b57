"""Applied forces, host side (no GPU): the header-derived binding of mjl_batch_attach_applied and
mjl_env_push, the argument errors reported before any device call, and the push rule's numpy restatement
(tests/applied_ref.py, the reference of the GPU test) on the library's generator (tests/rng_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import mjx_amd
from mjx_amd import _lib, abi
from mjx_amd._header import HEADER

from applied_ref import push_step, push_uniforms
from rng_ref import uniform01


def test_binding_has_the_headers_argument_lists():
    by_name = {n: (r, a) for r, n, a in HEADER.protos}
    assert by_name["mjl_batch_attach_applied"] == ("int", ["mjlBatch*", "float*", "float*"])
    assert by_name["mjl_env_push"] == ("int", ["mjlBatch*", "int", "int32_t*", "int", "int", "int", "float", "float",
                                               "float*", "uint64_t", "uint64_t", "float*", "void*"])
    assert "mjl_batch_attach_applied" in _lib.EXPORTS and "mjl_env_push" in _lib.EXPORTS
    L = _lib.lib()
    vp, i32, f32, u64 = C.c_void_p, C.c_int, C.c_float, C.c_uint64
    assert L.mjl_batch_attach_applied.argtypes == [vp, vp, vp] and L.mjl_batch_attach_applied.restype is i32
    assert L.mjl_env_push.argtypes == [vp, i32, vp, i32, i32, i32, f32, f32, vp, u64, u64, vp, vp]
    assert L.mjl_env_push.restype is i32


def test_null_batch_is_an_argument_error_without_gpu():
    L = _lib.lib()
    err = HEADER.enums["MJL_ERR_ARG"]
    assert L.mjl_batch_attach_applied(None, None, None) == err
    assert b"null batch" in L.mjl_last_error()
    assert L.mjl_env_push(None, 1, None, 1, 2, 1, 0.0, 1.0, None, 0, 0, None, None) == err
    assert b"null batch" in L.mjl_last_error()


def test_no_field_was_added():
    assert len(abi.FIELD) == 16 and HEADER.enums["MJL_NFIELD"] == 16


def test_push_stream_is_the_librarys_generator_with_the_push_tag():
    seed, counter = 0x1234_5678_9ABC_DEF0, 41
    u = push_uniforms(seed, counter, 5)
    assert u.shape == (5, 3) and u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    for e in (0, 4):
        for i in range(3):
            assert u[e, i] == uniform01(seed, counter ^ (1 << 62), np.uint64(e), np.uint64(i))
    # off the reset stream (same counter, no tag) and the pool stream (tag 2^63)
    assert not np.array_equal(u[:, 0], uniform01(seed, counter, np.arange(5, dtype=np.uint64), np.zeros(5, np.uint64)))
    assert not np.array_equal(u, push_uniforms(seed, counter + 1, 5))


def test_push_rule_restatement():
    """The schedule on the generator's draws: a push lasts `duration` calls, the gaps between pushes are the
    drawn intervals (within lo..hi), the force is horizontal with magnitude in the range, and `done` ends a
    push and redraws the interval."""
    nenv, interval, duration, force = 6, (3, 5), 2, (20.0, 60.0)
    timer, row = np.zeros((nenv, 2), np.int32), np.zeros((nenv, 6), np.float32)
    starts = [[] for _ in range(nenv)]
    for t in range(60):
        before = timer.copy()
        push_step(timer, row, push_uniforms(7, t + 1, nenv), None, interval, duration, force)
        on = np.abs(row).sum(1) > 0
        for e in range(nenv):
            if timer[e, 0] == duration and before[e, 0] == 0:
                starts[e].append(t)
                assert 20.0 <= np.hypot(row[e, 0], row[e, 1]) <= 60.0 * (1 + 1e-6) and not row[e, 2:].any()
            assert (timer[e, 0] > 0) == on[e]
            assert 1 <= timer[e, 1] <= interval[1]
    for e in range(nenv):
        gaps = np.diff(starts[e])  # a push holds for `duration` calls after the one that starts it
        assert len(gaps) > 5 and (gaps >= duration + interval[0]).all() and (gaps <= duration + interval[1]).all()
        assert len(set(gaps)) > 1
    # done: the row is cleared, the timer holds (0, a fresh draw) whatever it held
    timer[:] = (2, 1)
    row[:] = 1.0
    done = np.array([1, 0, 1, 0, 0, 1], np.float32)
    u = push_uniforms(7, 99, nenv)
    push_step(timer, row, u, done, interval, duration, force)
    for e in range(nenv):
        if done[e] > 0.5:
            assert not row[e].any() and timer[e, 0] == 0
            assert timer[e, 1] == interval[0] + min(int(np.floor(u[e, 0] * np.float32(3))), 2)
        else:
            assert row[e].all() and tuple(timer[e]) == (1, 1)


def test_train_ppo_push_flags():
    """--push-* reach PPOTrainer's `push`; without them the trainer gets None (today's path)."""
    import train_ppo
    from mjx_amd.config import reference_ppo_config
    from mjx_amd.envs import resolve_ids
    m = mjx_amd.load_model("humanoid_mjx")
    ecfg = resolve_ids(m, reference_ppo_config().env_config)
    assert train_ppo.push_config(train_ppo.parse_args([]), m, ecfg) is None
    a = train_ppo.parse_args(["--push-force", "100", "300"])
    assert train_ppo.push_config(a, m, ecfg) == {"body": ecfg.pelvis_body_id, "interval": (100, 200), "duration": 5,
                                                  "force": (100.0, 300.0)}
    a = train_ppo.parse_args(["--push-force", "50", "80", "--push-interval", "2", "4", "--push-duration", "3",
                              "--push-body", "torso"])
    assert train_ppo.push_config(a, m, ecfg) == {"body": m.name2id("body", "torso"), "interval": (2, 4), "duration": 3,
                                                  "force": (50.0, 80.0)}
    with pytest.raises(SystemExit):
        train_ppo.parse_args(["--push-body", "torso"])  # needs --push-force
    with pytest.raises(SystemExit):
        train_ppo.push_config(train_ppo.parse_args(["--push-force", "1", "2", "--push-body", "nobody"]), m, ecfg)
