"""Ray patterns for `mjx.ray_scan` / `HumanoidEnv.scan`: (lpnt, lvec) pairs of float32 [nray, 3] arrays in the
carrying frame (x forward, y left, z up), directions of unit length so that distances come back in metres."""
from __future__ import annotations

import numpy as np


def grid_pattern(nx: int, ny: int, dx: float, dy: float, height: float):
    """A height scanner: nx x ny downward rays (vec = -z) from `height` metres above the frame origin, spaced dx
    along x and dy along y and centred on the origin; ray i * ny + j is column i (x), row j (y). With
    align="yaw" the grid follows the heading and stays level, and `height - dist` is the terrain height under
    each point relative to the frame origin."""
    if nx < 1 or ny < 1:
        raise ValueError("grid_pattern needs nx, ny >= 1")
    x = (np.arange(nx) - 0.5 * (nx - 1)) * dx
    y = (np.arange(ny) - 0.5 * (ny - 1)) * dy
    gx, gy = np.meshgrid(x, y, indexing="ij")
    lpnt = np.stack([gx.ravel(), gy.ravel(), np.full(nx * ny, float(height))], axis=1)
    lvec = np.tile([0.0, 0.0, -1.0], (nx * ny, 1))
    return lpnt.astype(np.float32), lvec.astype(np.float32)


def fan_pattern(n: int, fov_deg: float, elevation_deg: float = 0.0):
    """A planar lidar: n rays from the frame origin, azimuths spread evenly over fov_deg about +x (from
    -fov / 2 to +fov / 2, ends included; one ray: +x; a 360 degree fan leaves the duplicate end out), all raised
    by elevation_deg above the frame's xy plane."""
    if n < 1:
        raise ValueError("fan_pattern needs n >= 1")
    if n == 1:
        az = np.zeros(1)
    elif fov_deg >= 360.0:
        az = np.deg2rad(-180.0 + 360.0 * np.arange(n) / n)
    else:
        az = np.deg2rad(np.linspace(-0.5 * fov_deg, 0.5 * fov_deg, n))
    el = np.deg2rad(elevation_deg)
    lvec = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.full(n, np.sin(el))], axis=1)
    return np.zeros((n, 3), np.float32), lvec.astype(np.float32)
