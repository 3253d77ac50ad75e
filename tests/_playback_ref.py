"""float64 numpy restatements of the two playback kernels (csrc/playback.hip; include/harp_hip.h says what they compute):
harp_motion_resample and harp_resolve_u8.  The yardstick of tests/test_gpu_avatar_player.py; tests/test_playback_cpu.py shows that its
slerp is the geodesic of rotation matrices."""
import numpy as np


def quat_of(a):
    """axis-angle (...,3) -> unit quaternion (...,4), w first"""
    a = np.asarray(a, np.float64)
    t = np.linalg.norm(a, axis=-1, keepdims=True)
    s = np.where(t < 1e-8, 0.5 - t * t / 48.0, np.sin(0.5 * t) / np.where(t < 1e-8, 1.0, t))
    return np.concatenate([np.cos(0.5 * t), s * a], -1)


def quat_to_matrix(q):
    w, x, y, z = np.moveaxis(np.asarray(q, np.float64), -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def rotation_matrix(a):
    return quat_to_matrix(quat_of(a))


def slerp(q0, q1, f):
    """shortest-arc spherical interpolation of unit quaternions (...,4) at f (...,): a slerp everywhere (no nlerp branch); where the two
    coincide to 1e-12 the weights' limit (1 - f, f)"""
    q0, q1, f = np.asarray(q0, np.float64), np.asarray(q1, np.float64), np.asarray(f, np.float64)[..., None]
    d = (q0 * q1).sum(-1, keepdims=True)
    q1 = np.where(d < 0, -q1, q1)
    d = np.abs(d)
    # the angle from atan2(|q0 - q1| |q0 + q1| / 2, d): accurate where acos(d) is not (d -> 1)
    so = np.minimum(0.5 * np.linalg.norm(q0 - q1, axis=-1, keepdims=True) * np.linalg.norm(q0 + q1, axis=-1, keepdims=True), 1.0)
    om = np.arctan2(so, d)
    tiny = so < 1e-12
    den = np.where(tiny, 1.0, so)
    s0 = np.where(tiny, 1.0 - f, np.sin((1.0 - f) * om) / den)
    s1 = np.where(tiny, f, np.sin(f * om) / den)
    q = s0 * q0 + s1 * q1
    return q / np.linalg.norm(q, axis=-1, keepdims=True)


def motion_resample(keys, n_rot, times, rot_offset=None):
    """keys (Tk, 3 n_rot + n_lin) float32, times (Tn,) float32 -> (rows, R, lin): for every output row the key row it must EQUAL bit for
    bit (or -1), the float64 rotation matrices (Tn, n_rot, 3, 3) of (resampled triple + offset) and the float64 linear channels (Tn, n_lin)"""
    keys32, times32 = np.asarray(keys, np.float32), np.asarray(times, np.float32)
    Tk, W = keys32.shape
    off = np.zeros(3 * n_rot) if rot_offset is None else np.asarray(rot_offset, np.float32).astype(np.float64)
    t = np.where(np.isnan(times32), np.float32(0), times32)
    t = np.minimum(np.maximum(t, np.float32(0)), np.float32(Tk - 1)).astype(np.float64)
    k = np.maximum(np.minimum(t.astype(np.int64), Tk - 2), 0)
    f = t - k
    rows = np.where(f == 0, k, np.where(f == 1, k + 1, -1))
    k1 = np.minimum(k + 1, Tk - 1)
    K = keys32.astype(np.float64)
    a = (K[:, :3 * n_rot] + off).reshape(Tk, n_rot, 3)
    q = slerp(quat_of(a[k]), quat_of(a[k1]), np.broadcast_to(f[:, None], (len(t), n_rot)))
    lin = (1.0 - f)[:, None] * K[k, 3 * n_rot:] + f[:, None] * K[k1, 3 * n_rot:]
    return rows, quat_to_matrix(q), lin


def ambiguous_pairs(keys, n_rot, rot_offset=None):
    """smallest |q0 . q1| over neighbouring key rows: below 1e-3 the relative rotation is within 0.12 degrees of 180 and every slerp's
    choice of arc is decided by rounding"""
    K = np.asarray(keys, np.float32).astype(np.float64)
    if n_rot == 0 or K.shape[0] < 2:
        return 1.0
    off = np.zeros(3 * n_rot) if rot_offset is None else np.asarray(rot_offset, np.float32).astype(np.float64)
    q = quat_of((K[:, :3 * n_rot] + off).reshape(K.shape[0], n_rot, 3))
    return float(np.abs((q[:-1] * q[1:]).sum(-1)).min())


def quantise(v):
    return np.clip(np.floor(255.0 * v + 0.5), 0, 255).astype(np.int64)


def resolve_u8(rgb, face_id, ss, bg=None, bg_rows=None, bg_color=(1.0, 1.0, 1.0), channels=3):
    """-> dict(out (B,S,S,channels) uint8, v255 (B,S,S,3) float64 = 255 v before rounding, n (B,S,S) covered sub-pixels)"""
    rgb, face_id = np.asarray(rgb, np.float32).astype(np.float64), np.asarray(face_id)
    B, Sh = face_id.shape[:2]
    S, N = Sh // ss, ss * ss
    color_b = quantise(np.fmin(np.fmax(np.asarray(bg_color, np.float32).astype(np.float64), 0.0), 1.0))
    back = np.broadcast_to(color_b, (B, S, S, 3)).copy()
    if bg is not None:
        bg = np.asarray(bg)
        n_bg = bg.shape[0]
        rows = np.asarray(bg_rows) if bg_rows is not None else (np.arange(B) if n_bg == B else np.zeros(B, np.int64))
        for b in range(B):
            if 0 <= rows[b] < n_bg:
                back[b] = bg[rows[b]]
    cov = (face_id >= 0).reshape(B, S, ss, S, ss)
    n = cov.sum((2, 4))
    c = np.fmin(np.fmax(rgb, 0.0), 1.0).reshape(B, S, ss, S, ss, 3)          # (fmax / fmin ignore a NaN: it becomes 0)
    tot = (c * cov[..., None]).sum((2, 4))
    v255 = 255.0 * (tot + (N - n)[..., None] * (back / 255.0)) / N
    col = np.where((n == 0)[..., None], back, np.clip(np.floor(v255 + 0.5), 0, 255).astype(np.int64))
    out = col if channels == 3 else np.concatenate([col, ((255 * n + N // 2) // N)[..., None]], -1)
    return dict(out=out.astype(np.uint8), v255=v255, n=n)
