"""float64 numpy restatement of harp_motion_filter (csrc/filter.hip; include/harp_hip.h states the contract): the same algorithm, the same
fixed number of iterations, the same order of the sums (the window is the leading axis of every array, and numpy reduces a leading axis
slice by slice: centre, t - 1, t + 1, t - 2, ...).  The yardstick of tests/test_gpu_filter.py; tests/test_filter_cpu.py shows that
two of its iterations reach the converged geodesic mean of rotation matrices.  Only the sample weights a_s = tap c_s are formed in
float32, as the contract defines them; which samples count is decided on the float32 inputs, everything after that is float64.

Besides the result it reports which (row, channel) cases float32 cannot decide (`undecidable`): a sign alignment with |dot| < 1e-3, a trim
distance within 1e-3 (relative) of its threshold, a chordal sum below 1e-3 sum a."""
import numpy as np

from tests._playback_ref import quat_of, quat_to_matrix

ALIGN_EPS = TRIM_EPS = CHORD_EPS = 1e-3


def qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - (av * bv).sum(-1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], -1)


def qconj(a):
    return a * np.array([1.0, -1.0, -1.0, -1.0])


def qlog(q):
    """rotation vector of q taken with w >= 0: 2 atan2(|v|, w) v / |v|"""
    q = np.where(q[..., :1] < 0, -q, q)
    vn = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    g = np.where(vn < 1e-300, 2.0, 2.0 * np.arctan2(vn, q[..., :1]) / np.where(vn < 1e-300, 1.0, vn))
    return g * q[..., 1:]


def _sanitise32(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isfinite(x) & (x > 0), x, np.float32(0)).astype(np.float32)


def window_radius(T, R, segment=None):
    """R_t (T,): the largest d <= R with every row t +- d' (d' <= d) inside [0, T) and in the segment of t"""
    seg = np.zeros(T, np.int64) if segment is None else np.asarray(segment).astype(np.int64)
    t = np.arange(T)
    Rt, alive = np.zeros(T, np.int64), np.ones(T, bool)
    for d in range(1, R + 1):
        ok = alive & (t - d >= 0) & (t + d < T)
        ok[ok] = (seg[t[ok] - d] == seg[t[ok]]) & (seg[t[ok] + d] == seg[t[ok]])
        Rt[ok] = d
        alive = ok
    return Rt


def _rot_mean(a, q, use, iters):
    """a (K,T,C) weights (0 where not used), q (K,T,C,4), use (K,T,C), at least one sample used per (T,C) that matters ->
    mu (T,C,4), degenerate (T,C), undecidable (T,C)"""
    kf = np.argmax(use, axis=0)                                       # the first used sample in visiting order
    qf = np.take_along_axis(q, kf[None, :, :, None], 0)[0]
    dots = (q * qf[None]).sum(-1)
    und = (use & (np.abs(dots) < ALIGN_EPS)).any(0)
    qa = np.where((dots < 0)[..., None], -q, q)
    sa = a.sum(0)
    S = (a[..., None] * qa).sum(0)
    nrm = np.linalg.norm(S, axis=-1)
    degenerate = nrm < 1e-6 * sa
    und |= nrm < CHORD_EPS * sa
    safe = np.where(nrm > 0, nrm, 1.0)
    mu = S / safe[..., None]
    mu = np.where((nrm > 0)[..., None], mu, np.array([1.0, 0, 0, 0]))
    sa1 = np.where(sa > 0, sa, 1.0)
    for _ in range(iters):
        l = qlog(qmul(qconj(mu)[None], q))
        v = (a[..., None] * l).sum(0) / sa1[..., None]
        mu = qmul(mu, quat_of(v))
    return mu, degenerate, und


def motion_filter(rows, n_rot, n_vec, taps, weights=None, segment=None, trim=None, rot_offset=None, iters=2):
    """rows (T, W) float32 -> dict(out (T, W) float64, used (T, nch) int, copy (T, nch) bool: the channel must equal the input bit for bit,
    R (T, n_rot, 3, 3): the rotation matrices of (out + offset), scale (T, nch): the largest magnitude among the used samples of the
    window (vector and scalar channels), undecidable (T, nch) bool)"""
    rows32 = np.asarray(rows, np.float32)
    T, W = rows32.shape
    n3 = n_rot + n_vec
    n_lin = W - 3 * n3
    nch = n3 + n_lin
    assert n_lin >= 0 and nch > 0
    taps32 = np.asarray(taps, np.float32).reshape(-1)
    R = taps32.shape[0] - 1
    Rt = window_radius(T, R, segment)
    K = 2 * R + 1
    dk = (np.arange(K) + 1) // 2                                      # 0 1 1 2 2 ...
    sk = np.where(np.arange(K) % 2 == 1, -dk, dk)                     # 0 -1 +1 -2 +2 ...
    inside = dk[:, None] <= Rt[None, :]                               # (K,T)
    Sc = np.clip(np.arange(T)[None, :] + sk[:, None], 0, T - 1)
    if weights is None:
        c = np.ones((T, nch), np.float32)
    else:
        c = np.asarray(weights, np.float32)
        c = np.broadcast_to(c.reshape(T, 1) if c.ndim == 1 else c, (T, nch))
    c = _sanitise32(c)
    with np.errstate(over="ignore", invalid="ignore"):
        a32 = _sanitise32(_sanitise32(taps32)[dk][:, None, None] * c[Sc])      # (K,T,nch): the float32 product
    vals = np.zeros((T, nch, 3), np.float32)
    vals[:, :n3] = rows32[:, :3 * n3].reshape(T, n3, 3)
    vals[:, n3:, 0] = rows32[:, 3 * n3:]
    finite = np.isfinite(vals).all(-1)
    use = inside[:, :, None] & (a32 > 0) & finite[Sc]
    a = np.where(use, a32.astype(np.float64), 0.0)
    V = np.where(use[..., None], vals[Sc].astype(np.float64), 0.0)    # (K,T,nch,3): an unused sample never enters arithmetic
    n = use.sum(0)
    tr = np.zeros(nch) if trim is None else np.asarray(trim, np.float32).astype(np.float64).reshape(nch)
    tr = np.where(tr > 0, tr, 0.0)                                    # (a NaN is not > 0)
    trimmed = tr > 0
    used = n.copy()
    und = np.zeros((T, nch), bool)
    out3 = np.zeros((T, nch, 3))

    # ---- vector and scalar channels
    sl = slice(n_rot, nch)
    if nch > n_rot:
        av, Vv, uv = a[:, :, sl], V[:, :, sl], use[:, :, sl]
        sa = av.sum(0)
        m = (av[..., None] * Vv).sum(0) / np.where(sa > 0, sa, 1.0)[..., None]
        dist = np.linalg.norm(Vv - m[None], axis=-1)
        thr = tr[sl][None, None, :]
        on = trimmed[sl][None, None, :]
        keep = uv & ~(on & (dist > thr))
        und[:, sl] |= (uv & on & (np.abs(dist - thr) <= TRIM_EPS * thr)).any(0)
        nk = keep.sum(0)
        redo = (nk > 0) & (nk < n[:, sl])
        ak = np.where(keep, av, 0.0)
        sk_ = ak.sum(0)
        m2 = (ak[..., None] * Vv).sum(0) / np.where(sk_ > 0, sk_, 1.0)[..., None]
        out3[:, sl] = np.where(redo[..., None], m2, m)
        used[:, sl] = np.where(redo, nk, n[:, sl])

    # ---- rotation channels
    Rm = np.zeros((T, n_rot, 3, 3))
    degenerate = np.zeros((T, nch), bool)
    off = np.zeros((n_rot, 3))
    if n_rot:
        if rot_offset is not None:
            off = np.asarray(rot_offset, np.float32).astype(np.float64).reshape(n_rot, 3)
        ar, ur = a[:, :, :n_rot], use[:, :, :n_rot]
        q = quat_of(V[:, :, :n_rot] + off)
        mu, deg, u1 = _rot_mean(ar, q, ur, iters)
        und[:, :n_rot] |= u1
        dist = np.linalg.norm(qlog(qmul(qconj(mu)[None], q)), axis=-1)
        thr = tr[:n_rot][None, None, :]
        on = trimmed[:n_rot][None, None, :] & ~deg[None]
        keep = ur & ~(on & (dist > thr))
        und[:, :n_rot] |= (ur & on & (np.abs(dist - thr) <= TRIM_EPS * thr)).any(0)
        nk = keep.sum(0)
        redo = (nk > 0) & (nk < n[:, :n_rot]) & ~deg
        mu2, deg2, u2 = _rot_mean(np.where(keep, ar, 0.0), q, keep, iters)
        mu = np.where(redo[..., None], mu2, mu)
        deg = np.where(redo, deg2, deg)
        und[:, :n_rot] |= redo & u2
        used[:, :n_rot] = np.where(deg, -1, np.where(redo, nk, n[:, :n_rot]))
        degenerate[:, :n_rot] = deg
        out3[:, :n_rot] = qlog(mu) - off
        Rm = quat_to_matrix(mu / np.linalg.norm(mu, axis=-1, keepdims=True))

    centre_only = (n == 1) & use[0]
    copy = (n == 0) | centre_only | degenerate
    used = np.where((n == 0) | centre_only, n, used)
    und &= ~((n == 0) | centre_only)
    src3 = vals.astype(np.float64)
    out3 = np.where(copy[..., None], src3, out3)
    if n_rot:
        with np.errstate(invalid="ignore"):
            Rm = np.where(copy[:, :n_rot, None, None], quat_to_matrix(quat_of(np.nan_to_num(src3[:, :n_rot]) + off)), Rm)
    out = np.concatenate([out3[:, :n3].reshape(T, 3 * n3), out3[:, n3:, 0]], 1)
    scale = np.abs(V).max((0, 3))
    return dict(out=out, used=used.astype(np.int64), copy=copy, R=Rm, scale=scale, undecidable=und, radius=Rt)
