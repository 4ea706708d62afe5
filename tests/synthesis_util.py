"""Float64 restatements for the synthesis tests (numpy only): lerp / slerp of the reference's utils/interp.py at the
float32 weights of torch.linspace(0, 1, n), the demo's view (demo.py:188-226 with utils/geometry.py:5-35) and an ordered
stream compaction (a boolean index in row-major order)."""
import numpy as np

# the seeded endpoint pairs of tests/golden/synthesis.npz (make_synthesis_golden.py) and the walks recorded from them
WALK_NZ = (1, 7, 100, 512)
WALK_N = (1, 2, 8)
# (zoom m, yaw deg, pitch deg): the demo's default first
VIEWS = ((60, -45, 60), (1, 180, 0), (120, -180, 90), (37, 13, 29), (90, 0, 45))


def linspace01(n):
    """torch.linspace(0, 1, n) in float32: step = 1 / (n - 1) in float32; the first half counts up from 0, the second down
    from 1 with one rounding (ATen RangeFactories: 1 - step k as a fused multiply-add; the float64 product of a float32
    and a small integer is exact, so rounding the float64 expression once is the same)"""
    n = int(n)
    if n == 1:
        return np.zeros(1, np.float32)
    step = np.float64(np.float32(1.0) / np.float32(n - 1))
    i = np.arange(n)
    return np.where(i < n // 2, (step * i).astype(np.float32), (1.0 - step * (n - 1 - i)).astype(np.float32))


def lerp(val, low, high):
    low, high = np.asarray(low, np.float64), np.asarray(high, np.float64)
    return low + (high - low) * np.float64(val)


def slerp(val, low, high):
    """the angle from the normalised endpoints, the un-normalised ones blended"""
    low, high, val = np.asarray(low, np.float64), np.asarray(high, np.float64), np.float64(val)
    with np.errstate(invalid="ignore", divide="ignore"):
        omega = np.arccos(np.sum((low / np.linalg.norm(low)) * (high / np.linalg.norm(high))))
        so = np.sin(omega)
        return (np.sin((1.0 - val) * omega) / so) * low + (np.sin(val * omega) / so) * high


def walk(z0, z1, n, mode):
    """[n, nz] float64: row i = mode(w_i, z0, z1), w = linspace01(n)"""
    f = {"lerp": lerp, "slerp": slerp}[mode]
    return np.stack([f(w, z0, z1) for w in linspace01(n)])


def rotation(angles):
    """utils/geometry.py:5-35: R = Rz Ry Rx of the radians (x, y, z), float64"""
    x, y, z = (np.float64(a) for a in angles)
    Rx = np.array([[1, 0, 0], [0, np.cos(x), -np.sin(x)], [0, np.sin(x), np.cos(x)]])
    Ry = np.array([[np.cos(y), 0, np.sin(y)], [0, 1, 0], [-np.sin(y), 0, np.cos(y)]])
    Rz = np.array([[np.cos(z), -np.sin(z), 0], [np.sin(z), np.cos(z), 0], [0, 0, 1]])
    return Rz @ (Ry @ Rx)


def view_angles(yaw_deg, pitch_deg):
    """demo.py:200-225: the radians (0, pitch, -yaw)"""
    return 0.0, pitch_deg / 180 * np.pi, -yaw_deg / 180 * np.pi


def view(zoom_m=60, yaw_deg=-45, pitch_deg=60):
    """-> (R [3,3], t [3]) float64"""
    z = zoom_m / 120.0
    return rotation(view_angles(yaw_deg, pitch_deg)), np.array([0.1 * z, 0.0, z])


def compact(points, valid):
    """points [B,3,H,W], valid [B,H,W] bool -> (records: a list of [k_b, 4] arrays, (x, y, z, 0) of the valid pixels in
    row-major order; counts [B])"""
    points, valid = np.asarray(points), np.asarray(valid, bool)
    B = points.shape[0]
    flat = points.reshape(B, 3, -1).transpose(0, 2, 1)
    records = []
    for b in range(B):
        xyz = flat[b][valid[b].reshape(-1)]
        records.append(np.concatenate([xyz, np.zeros((len(xyz), 1), xyz.dtype)], axis=1))
    return records, np.array([len(r) for r in records], np.int64)
