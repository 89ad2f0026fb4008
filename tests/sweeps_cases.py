"""The numpy oracle of the multi-sweep merge (include/sassd.h "Multi-sweep merge") and the seeded cases of its tests.  Written
from the contract, independently of sassd.stream.merge_sweeps_host: elementwise float64 numpy operations in the stated order,
one entry and one output row range at a time."""
import numpy as np

ST_POINT_OVERFLOW = 16


def merge_oracle(ring, slot, count, xform, T, dt, time_feature, cap_out):
    """ring [R, sweep_cap, ndim_in] f32, the descriptors as the kernel takes them -> (rows [n, ndim_out] f32, n, status flags)."""
    R, sweep_cap, nd = ring.shape
    nd_out = nd + (1 if time_feature else 0)
    parts, flag = [], 0
    for s in range(len(slot)):
        if int(count[s]) > sweep_cap:
            flag |= ST_POINT_OVERFLOW
        if not 0 <= int(slot[s]) < R:
            continue
        c = min(max(int(count[s]), 0), sweep_cap)
        src = ring[int(slot[s]), :c]
        rows = np.zeros((c, nd_out), np.float32)
        rows.view(np.uint32)[:, :nd] = src.view(np.uint32)                  # bit for bit
        if int(xform[s]) != 0:
            x, y, z = src[:, 0].astype(np.float64), src[:, 1].astype(np.float64), src[:, 2].astype(np.float64)
            for i in range(3):
                a = np.multiply(T[s, i, 0], x)
                b = np.multiply(T[s, i, 1], y)
                c2 = np.multiply(T[s, i, 2], z)
                acc = np.add(a, b)
                acc = np.add(acc, c2)
                acc = np.add(acc, T[s, i, 3])
                rows[:, i] = acc.astype(np.float32)
        if time_feature:
            rows[:, nd] = np.float32(dt[s])
        parts.append(rows)
    merged = np.concatenate(parts, 0) if parts else np.zeros((0, nd_out), np.float32)
    if len(merged) > cap_out:
        flag |= ST_POINT_OVERFLOW
    n = min(len(merged), cap_out)
    return np.ascontiguousarray(merged[:n]), n, flag


def merge_entries_oracle(entries, time_feature):
    """entries: (points [n, ndim_in] f32, T [3,4] f64 or None, dt) in entry order -> the merged cloud, through merge_oracle on a
    ring that holds one entry per slot."""
    cap = max(1, max(len(p) for p, _, _ in entries))
    nd = entries[0][0].shape[1]
    S = len(entries)
    ring = np.zeros((S, cap, nd), np.float32)
    T = np.zeros((S, 3, 4))
    for s, (p, t, _) in enumerate(entries):
        ring[s, :len(p)] = p
        if t is not None:
            T[s] = t
    rows, n, flag = merge_oracle(ring, np.arange(S), np.array([len(p) for p, _, _ in entries]),
                                 np.array([0 if t is None else 1 for _, t, _ in entries]), T,
                                 np.array([d for _, _, d in entries], np.float32), time_feature, S * cap)
    assert flag == 0 and n == sum(len(p) for p, _, _ in entries)
    return rows


def rigid_pose(yaw, pitch, roll, t):
    """sensor-to-world 4x4 float64: Rz(yaw) Ry(pitch) Rx(roll), translation t"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.]])
    ry = np.array([[cp, 0, sp], [0, 1., 0], [-sp, 0, cp]])
    rx = np.array([[1., 0, 0], [0, cr, -sr], [0, sr, cr]])
    out = np.eye(4)
    out[:3, :3] = rz @ ry @ rx
    out[:3, 3] = t
    return out


def seeded_pose(seed):
    g = np.random.default_rng(seed)
    return rigid_pose(g.uniform(-3, 3), g.uniform(-0.3, 0.3), g.uniform(-0.3, 0.3), g.uniform(-50, 50, 3))


def seeded_transform(seed):
    """[3,4] float64: a seeded rigid transform between two seeded poses, by the matrix product"""
    return (invert_rigid(seeded_pose(seed)) @ seeded_pose(seed + 1000))[:3]


def trajectory(n, seed=0, dt=0.05):
    """n poses of a seeded smooth drive (about 8 m/s along a gentle curve, small pitch and roll) and their times, `dt` apart"""
    g = np.random.default_rng(seed)
    yaw_rate, wob = g.uniform(0.1, 0.3), g.uniform(0.002, 0.01, 2)
    poses, pos, t0 = [], np.zeros(3), g.uniform(10, 20)
    for i in range(n):
        yaw = yaw_rate * dt * i
        poses.append(rigid_pose(yaw, wob[0] * np.sin(0.7 * i), wob[1] * np.cos(0.5 * i), pos.copy()))
        pos = pos + 8.0 * dt * np.array([np.cos(yaw), np.sin(yaw), 0.01])
    return poses, [t0 + dt * i for i in range(n)]


def invert_rigid(p):
    out = np.eye(4)
    out[:3, :3] = p[:3, :3].T
    out[:3, 3] = -(p[:3, :3].T @ p[:3, 3])
    return out


def sweeps_of_a_static_scene(cloud, poses):
    """Cut `cloud` [n, 4] f32 -- a static scene in the frame of poses[0] -- into len(poses) interleaved parts; part j is what
    the sensor at poses[j] sees of it: its xyz moved into that sensor frame (float64, rounded to float32), intensity kept."""
    n, w = len(poses), poses[0]
    out = []
    for j, pose in enumerate(poses):
        part = np.ascontiguousarray(cloud[j::n]).copy()
        m = invert_rigid(pose) @ w
        xyz = part[:, :3].astype(np.float64) @ m[:3, :3].T + m[:3, 3]
        part[:, :3] = xyz.astype(np.float32)
        out.append(part)
    return out


def frame_entries(sweeps, poses, times, t, S, start=0):
    """the entries of frame t of a sequence that started at sweep `start`: the current sweep, then up to S-1 earlier ones, newest
    first, with the transform the stream's contract names: inv(pose_t) @ pose_j, in float64"""
    from sassd.stream import sweep_transform
    ent = [(sweeps[t], None, 0.0)]
    for j in range(t - 1, max(start, t - S + 1) - 1, -1):
        ent.append((sweeps[j], sweep_transform(poses[t], poses[j]), np.float32(times[t] - times[j])))
    return ent
