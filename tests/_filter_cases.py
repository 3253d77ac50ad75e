"""The fixtures of the motion-filter tests (csrc/filter.hip), shared by tests/test_gpu_filter.py (the kernel against the yardstick of
tests/_filter_ref.py) and tests/test_filter_cpu.py (the yardstick alone: the share of float32-undecidable cases stays under the cap).
Seeded numpy only: no device, no library.

The data are built so that float32 can decide them: a channel's samples stay within 0.08 of their track (a bounded noise of at most
0.04 around a drift of amplitude 0.02), which is <= 0.5 x the trim threshold of 0.2, and the designed spikes of 0.7 are >= 2 x it; the
rotations of a window are close together, so no sign alignment is near a dot product of 0 and no chordal sum vanishes."""
import numpy as np

TS = (1, 2, 3, 7, 64, 257)                      # 257 x 1 channel crosses the 256-lane block; x 22 channels the blocks end in the middle of a row
RS = (0, 1, 3, 64)
MIXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (17, 2, 3), (0, 21, 0))
ANGLES = (0.0, 1e-9, 1e-5, np.pi - 1e-3, 4.0, 6.0)
TRIM = 0.2                                      # radians and vector units
NOISE, DRIFT, SPIKE = 0.04, 0.02, 0.7
MAX_UNDECIDABLE = 0.02


def gaussian(sigma, R):
    return [float(np.exp(-0.5 * (d / sigma) ** 2)) for d in range(R + 1)]


def _ball(rng, shape, radius):
    u = rng.normal(size=shape + (3,))
    return u / np.linalg.norm(u, axis=-1, keepdims=True) * (radius * rng.uniform(0.0, 1.0, size=shape + (1,)) ** (1.0 / 3.0))


def complement(aa):
    """the same rotations written with the angle minus 2 pi (triples below 1e-3 rad are left alone)"""
    th = np.linalg.norm(aa, axis=-1, keepdims=True)
    return np.where(th > 1e-3, aa * (th - 2.0 * np.pi) / np.where(th > 1e-3, th, 1.0), aa)


def make_rows(rng, T, n_rot, n_vec, n_lin, offset):
    """(T, W) float32: per rotation channel a base angle from ANGLES about a random axis (of triple + offset), a slow drift, a bounded
    noise of one of three sizes (none, 1e-6 of it, all of it), on every second channel frames that alternate with the 2 pi complement;
    vectors and scalars alike around a base within 0.3; two one-frame spikes per channel when the clip is long enough"""
    t = np.arange(T)[:, None, None]
    phase = rng.uniform(0, 2 * np.pi, size=(1, n_rot + n_vec + n_lin, 1))
    drift = DRIFT * np.sin(2 * np.pi * t / 97.0 + phase)
    scale = np.array([0.0, 1e-6, 1.0])[rng.integers(0, 3, size=n_rot + n_vec + n_lin)]
    scale[: min(3, scale.shape[0])] = (1.0, 0.0, 1e-6)[: min(3, scale.shape[0])]
    parts = []
    if n_rot:
        axis = rng.normal(size=(n_rot, 3))
        axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
        base = axis * np.array([ANGLES[(k + T) % len(ANGLES)] for k in range(n_rot)])[:, None]
        aa = base[None] + drift[:, :n_rot] * axis[None] + _ball(rng, (T, n_rot), NOISE) * scale[None, :n_rot, None]
        for s in _spikes(rng, T):
            aa[s] += axis * SPIKE * rng.choice([-1.0, 1.0], size=(n_rot, 1))      # about the channel's own axis: 0.7 rad as a rotation too
        alt = (np.arange(n_rot) % 2 == 1)[None, :, None] & (np.arange(T) % 2 == 1)[:, None, None]
        aa = np.where(alt, complement(aa), aa)
        parts.append((aa - offset.reshape(1, n_rot, 3)).reshape(T, 3 * n_rot))
    if n_vec:
        v = rng.uniform(-0.3, 0.3, size=(1, n_vec, 3)) + drift[:, n_rot:n_rot + n_vec] + _ball(rng, (T, n_vec), NOISE) * scale[None, n_rot:n_rot + n_vec, None]
        for s in _spikes(rng, T):
            v[s] += _unit(rng, n_vec) * SPIKE
        parts.append(v.reshape(T, 3 * n_vec))
    if n_lin:
        x = rng.uniform(-0.3, 0.3, size=(1, n_lin)) + drift[:, n_rot + n_vec:, 0] + rng.uniform(-NOISE, NOISE, size=(T, n_lin)) * scale[None, n_rot + n_vec:]
        for s in _spikes(rng, T):
            x[s] += SPIKE * rng.choice([-1.0, 1.0], size=n_lin)
        parts.append(x)
    return np.concatenate(parts, 1).astype(np.float32)


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=-1, keepdims=True)


def _spikes(rng, T):
    return [] if T < 7 else [int(s) for s in rng.choice(np.arange(1, T - 1), size=2 if T < 100 else 4, replace=False)]


def make_weights(rng, T, nch, R, per_channel):
    """confidences in (0.2, 1) with zeros, negatives, NaN and inf among them, and one gap of zeros longer than the window"""
    w = rng.uniform(0.2, 1.0, size=(T, nch) if per_channel else (T,)).astype(np.float32)
    bad = rng.uniform(size=w.shape) < 0.12
    w[bad] = rng.choice(np.array([0.0, -1.0, np.nan, np.inf, -np.inf], np.float32), size=int(bad.sum()))
    gap = 2 * R + 3
    if T >= gap + 2:
        lo = int(rng.integers(1, T - gap))
        w[lo:lo + gap] = 0.0
    return w


def make_segments(rng, T):
    """clip ids that change at random rows, single-row segments among them; the ids are not sorted"""
    cut = rng.uniform(size=T) < 0.15
    cut[0] = False
    if T >= 5:
        cut[2] = cut[3] = True                                          # row 2 is a segment of its own
    ids = rng.permutation(T + 3).astype(np.int32)
    return ids[np.cumsum(cut)]


def yardstick_cases(mix):
    """every (T, R) of TS x RS for one channel mix; the other switches — weights none / per row / per channel, segments, offset, iters 0 / 2,
    trim — cycle with co-prime periods so that each value meets each size"""
    n_rot, n_vec, n_lin = mix
    nch = n_rot + n_vec + n_lin
    k = 0
    for T in TS:
        for R in RS:
            rng = np.random.default_rng(1000 * T + 10 * R + nch)
            offset = rng.normal(size=3 * n_rot) * 0.2 if (k % 2 == 0 and n_rot) else np.zeros(3 * n_rot)
            rows = make_rows(rng, T, n_rot, n_vec, n_lin, offset)
            if n_vec and T >= 3:                                        # a non-finite coordinate is an unused sample
                rows[T // 2, 3 * n_rot] = np.nan
            wmode = k % 3
            yield dict(name=f"T{T}_R{R}_w{wmode}_k{k}", rows=rows, n_rot=n_rot, n_vec=n_vec, taps=gaussian(max(R / 2.0, 0.5), R),
                       weights=None if wmode == 0 else make_weights(rng, T, nch, R, wmode == 2),
                       segment=make_segments(rng, T) if k % 5 in (1, 3) else None,
                       trim=np.full(nch, TRIM, np.float32) * (np.arange(nch) % 4 != 3) if k % 2 == 1 or k % 7 == 0 else None,
                       rot_offset=offset.astype(np.float32) if (k % 2 == 0 and n_rot) else None, iters=(2, 0, 2, 2)[k % 4])
            k += 1


def spike_track(seed=7, T=64):
    """test 5: a smooth rotation track (one channel), the same with 0.02 rad noise, and that with two one-frame spikes of about 1 rad"""
    rng = np.random.default_rng(seed)
    t = np.arange(T)[:, None]
    clean = np.array([[0.3, -0.2, 0.5]]) + 0.4 * np.sin(2 * np.pi * t / 48.0) * np.array([[1.0, 0.5, -0.3]]) + 0.01 * t * np.array([[0.0, 1.0, 0.0]])
    noisy = clean + rng.normal(size=(T, 3)) * 0.02
    spiky = noisy.copy()
    for s, sg in ((17, 1.0), (41, -1.0)):
        spiky[s] += sg * np.array([0.6, -0.6, 0.5])
    return clean.astype(np.float32), noisy.astype(np.float32), spiky.astype(np.float32)
