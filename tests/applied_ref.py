"""numpy restatement of the push rule of mjl_env_push (include/mjx355.h), for tests.

float32 where the kernel is float32: the uniforms, the interval draw's product, the angle 2 pi u1 and the
magnitude; the timers are exact integers."""
import numpy as np

from rng_ref import uniform01

PUSH_TAG = 1 << 62  # the push stream's counter tag: uniform01(seed, counter ^ 2^62, env, i)
TWO_PI = np.float32(6.2831853071795864769)


def push_uniforms(seed: int, counter: int, nenv: int) -> np.ndarray:
    """The three uniforms of every env for one mjl_env_push call without `noise`, float32 [nenv, 3]."""
    env = np.repeat(np.arange(nenv, dtype=np.uint64), 3)
    idx = np.tile(np.arange(3, dtype=np.uint64), nenv)
    return uniform01(seed, (counter ^ PUSH_TAG) & 0xFFFFFFFFFFFFFFFF, env, idx).reshape(nenv, 3)


def push_step(timer: np.ndarray, row: np.ndarray, u: np.ndarray, done, interval, duration: int, force) -> None:
    """One call, in place: timer int32 [nenv, 2] = (steps_left, steps_to_next), row float32 [nenv, 6] the
    pushed body's xfrc row, u float32 [nenv, 3], done [nenv] or None."""
    lo, hi = int(interval[0]), int(interval[1])
    flo, fhi = np.float32(force[0]), np.float32(force[1])
    u = np.asarray(u, np.float32)
    for e in range(timer.shape[0]):
        span = hi - lo
        nxt = lo + min(int(np.floor(u[e, 0] * np.float32(span + 1))), span)
        if done is not None and done[e] > 0.5:
            row[e] = 0
            timer[e] = (0, nxt)
        elif timer[e, 0] > 0:
            timer[e, 0] -= 1
            if timer[e, 0] == 0:
                row[e] = 0
        else:
            timer[e, 1] -= 1
            if timer[e, 1] <= 0:
                th = TWO_PI * u[e, 1]
                F = np.float32(flo + u[e, 2] * np.float32(fhi - flo))
                row[e] = (F * np.cos(th), F * np.sin(th), 0, 0, 0, 0)
                timer[e] = (duration, nxt)
