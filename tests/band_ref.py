"""The narrow-band SDF sweep in plain numpy - the reference tests/test_gpu_mesh_band.py holds csrc/mesh_band.hip and mesh_util.banded_volume to.

It works on a DENSE volume: the banded values at the points of active bricks ARE the dense values and the fill of an inactive brick IS the dense
value at its probe point, so the reference needs no SDF of its own.  The method:

  * grid points (i, j, k) in 0 .. N - 1; brick (bx, by, bz) owns the points with i // B == bx, j // B == by, k // B == bz; nb = ceil(N / B) per
    axis, the last ragged when N % B != 0; linear brick index (bx nb + by) nb + bz;
  * probe of a brick: the grid point min(b B + B // 2, N - 1) per axis;
  * band test: active iff NOT (|f(probe) - level| > threshold), in float32 (a NaN probe is active);
    threshold = float32(lipschitz * sqrt(3) * max(B // 2 + 1, B - B // 2) * volume_size / (N - 1)), the product taken in double;
  * check: over all grid edges (toward +x, +y, +z), inside iff value < level: an edge whose ends differ and that has an end in an inactive brick
    makes that brick wanted; wanted bricks are activated and the check runs again, at most max_rounds times; bricks still wanted after that:
    every remaining brick is activated (completed_dense).
"""
import numpy as np


def n_bricks_axis(N, B):
    return -(-N // B)


def brick_of(N, B):
    """[N, N, N] int64: the linear brick index of every grid point."""
    nb = n_bricks_axis(N, B)
    b = np.arange(N) // B
    return (b[:, None, None] * nb + b[None, :, None]) * nb + b[None, None, :]


def probe_index(N, B):
    """[nb] the probe's grid index per brick coordinate."""
    return np.minimum(np.arange(n_bricks_axis(N, B)) * B + B // 2, N - 1)


def probe_values(dense, B):
    """[nb^3] float32: the dense volume at the probe points, in brick order."""
    p = probe_index(dense.shape[0], B)
    return np.ascontiguousarray(dense[np.ix_(p, p, p)], dtype=np.float32).reshape(-1)


def threshold(N, volume_size, B, lipschitz):
    reach_steps = max(B // 2 + 1, B - B // 2)
    return np.float32(float(lipschitz) * (np.sqrt(3.0) * reach_steps * (volume_size / (N - 1))))


def wanted_bricks(vol, level, active, bricks):
    """[nb^3] bool: the inactive bricks that hold an end of an edge of vol whose ends differ in `value < level`."""
    inside = vol < np.float32(level)
    want = np.zeros(active.shape, dtype=bool)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = inside[lo] != inside[hi]
        want[bricks[lo][cross]] = True
        want[bricks[hi][cross]] = True
    return want & ~active


def banded(dense, B, level, thr, max_rounds=4):
    """dense [N, N, N] float32 -> (vol, masks, info): the banded volume, the list of per-round masks of NEWLY active bricks ([nb^3] bool: the probe
    test's, one per repair round, the dense completion's if it ran) and the counts mesh_util.banded_volume reports."""
    dense = np.ascontiguousarray(dense, dtype=np.float32)
    N = dense.shape[0]
    assert dense.shape == (N, N, N) and 2 <= B <= 64
    bricks = brick_of(N, B)
    points_of = np.bincount(bricks.reshape(-1))
    probe = probe_values(dense, B)
    with np.errstate(invalid="ignore"):
        first = ~(np.abs(probe - np.float32(level)) > np.float32(thr))
    active = first.copy()
    masks = [first]
    vol = np.where(active[bricks], dense, probe[bricks]).astype(np.float32)
    rounds, completed = 0, False
    while True:
        want = wanted_bricks(vol, level, active, bricks)
        if not want.any():
            break
        if rounds < max_rounds:
            rounds += 1
        else:
            want = ~active
            completed = True
        masks.append(want)
        active = active | want
        vol = np.where(active[bricks], dense, vol).astype(np.float32)
        if completed:
            break
    info = {"bricks": int(active.size), "active": [int(m.sum()) for m in masks], "evaluated_points": int(sum(points_of[m].sum() for m in masks)),
            "repair_rounds": rounds, "completed_dense": completed, "threshold": float(np.float32(thr))}
    return vol, masks, info
