"""TEST INFRASTRUCTURE ONLY — the synthetic meshes of tests/test_gpu_raster_paths.py (given directly as NDC vertices) and, per case, the
conditions that make it force its path, asserted on the float64 restatement (tests/_raster_ref.py) alone: tests/test_raster_ref_cpu.py
runs them without a GPU, the GPU tests run them again on the reference they compare with."""
import math

import numpy as np
import torch

from tests import _raster_ref as R

SIGMA = 1e-4                                           # band sqrt(blur) = 0.030 NDC: about half a pixel at S = 32 .. 96
BLUR = math.log(9999.0) * SIGMA
K_STAGE, CAP2 = 256, 128                               # raster_body.h: kStage, RASTER_CAP2
CASES = ("one_face", "fan", "many_faces", "layers", "culled", "empty_frame", "moves_a", "moves_b", "order")
WORKLOAD = ("one_face_w", "fan_w")                     # the same meshes with one edge inside the workload's band of a pixel row


def yc(i, S):
    return 1.0 - (2.0 * i + 1.0) / S


def _bump(x, y, amp):
    return amp * np.sin(3.0 * x + 0.3) * np.cos(2.0 * y + 0.7)


def grid(nx, ny, x0, x1, y0, y1, z=1.5, amp=0.05):
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    X, Y = np.meshgrid(xs, ys)
    v = np.stack([X, Y, z + _bump(X, Y, amp)], -1).reshape(-1, 3)
    a = (np.arange(ny)[:, None] * (nx + 1) + np.arange(nx)[None, :]).reshape(-1)
    b, c, d = a + 1, a + nx + 2, a + nx + 1
    return v, np.concatenate([np.stack([a, c, b], 1), np.stack([a, d, c], 1)], 0).astype(np.int64)


def join(*meshes):
    vs, fs, off = [], [], 0
    for v, f in meshes:
        vs.append(v)
        fs.append(f + off)
        off += v.shape[0]
    return np.concatenate(vs), np.concatenate(fs)


def fan(n, centre, radius, spoke_y=None):
    ang = 2 * np.pi * (np.arange(n) + 0.37) / n
    rr = radius * (1.0 + 0.11 * np.sin(7 * ang + 0.3))
    rim = np.stack([centre[0] + rr * np.cos(ang), centre[1] + rr * np.sin(ang), 1.45 + 0.1 * np.sin(3 * ang)], -1)
    if spoke_y is not None:
        rim[0, 1] = spoke_y
    v = np.concatenate([np.array([[centre[0], centre[1], 1.5]]), rim], 0)
    k = np.arange(n)
    return v, np.stack([np.zeros(n, np.int64), 1 + (k + 1) % n, 1 + k], 1)


def build(name):
    """dict(name, S, B, ndc (B,V,3) float32, faces (F,3) int64, blur, sigma [, alone: the face rows of the `culled` case that can be seen])"""
    from harp_amd import ops
    sigma, blur = (ops.SIL_SIGMA, ops.SIL_BLUR) if name in WORKLOAD else (SIGMA, BLUR)
    extra = {}
    if name in ("one_face", "one_face_w"):
        S = 72
        t0 = np.array([[0.8731, 0.7919, 1.3], [-0.9127, 0.4733, 2.1], [0.1291, -0.8817, 1.7]])
        t1 = np.array([[-0.8431, -0.9019, 1.1], [0.9313, -0.2871, 1.9], [-0.3517, 0.9207, 2.4]])
        if name == "one_face_w":                       # edge 0-1 horizontal, 4.1e-4 NDC above the centres of pixel row 20 (band 9.6e-4)
            t0[0, 1] = t0[1, 1] = yc(20, S) + 4.1e-4
        v, f = np.stack([t0, t1]), np.array([[0, 1, 2]])
    elif name in ("fan", "fan_w"):
        S, n = 48, 613
        c0 = [0.0137, -0.0217]                         # (centres chosen so that none of the 613 band tests of a pixel near the hub is undecided)
        sy = None
        if name == "fan_w":                            # the spoke to rim vertex 0 horizontal, 3.7e-4 NDC above the centres of pixel row 24
            c0[1] = sy = yc(24, S) + 3.7e-4
        v0, f = fan(n, c0, 0.24, sy)
        v1, _ = fan(n, (0.3477, -0.3137), 0.19)
        v = np.stack([v0, v1])
    elif name == "many_faces":
        S = 64
        v, f = grid(66, 63, -0.9713, 0.9547, -0.9631, 0.9683, z=1.6, amp=0.1)
        v = v[None]
    elif name == "layers":
        S = 40
        sheets = (grid(5, 5, -0.83, 0.79, -0.77, 0.85, z=2.3), grid(4, 4, -0.55, 0.31, -0.43, 0.61, z=1.7), grid(3, 3, -0.13, 0.67, -0.71, 0.11, z=1.2))
        v, f = join(*sheets)
        ends = np.cumsum([m[1].shape[0] for m in sheets])
        spans = [(int(e - m[1].shape[0]), int(e)) for m, e in zip(sheets, ends)]          # face id range of each sheet
        front = spans[2][0]                            # first face of the front sheet
        tri = np.array([[-0.71, 0.33], [-0.23, 0.47], [-0.49, 0.79]])
        far = np.concatenate([tri, np.full((3, 1), 0.900001)], 1)
        near = np.concatenate([tri, np.full((3, 1), 0.9)], 1)
        nv = v.shape[0]
        v = np.concatenate([v, far, near], 0)
        # ... | the far one of the close pair | the near one (HIGHER id) | a copy of a front-sheet face (exact tie: the lower id wins)
        f = np.concatenate([f, [[nv, nv + 1, nv + 2]], [[nv + 3, nv + 4, nv + 5]], f[front + 4:front + 5]], 0)
        extra = dict(tie=(front + 4, f.shape[0] - 1), close=(f.shape[0] - 3, f.shape[0] - 2), sheets=spans)
        v = np.stack([v, v + np.array([0.0371, -0.0293, 0.0])])
    elif name == "culled":
        S = 40
        sv, sf = grid(6, 6, -0.71, 0.73, -0.6831, 0.7417, z=1.5)
        nan = float("nan")
        tris = dict(behind=[[-0.31, 0.22, -1.0], [0.43, 0.11, -1.5], [0.07, -0.52, -0.7]],
                    near_vertex=[[-0.41, -0.32, 1.2], [0.33, -0.21, 1e-9], [0.12, 0.47, 1.4]],
                    zero_area=[[-0.2, 0.1, 1.1], [-0.2, 0.1, 1.1], [0.3, 0.4, 1.2]],
                    nan=[[nan, 0.3, 1.2], [0.5, -0.4, 1.3], [-0.1, -0.6, 1.1]],
                    off_screen=[[1.6, -0.3, 1.3], [2.4, 0.1, 1.3], [1.9, 0.4, 1.3]],
                    crossing=[[0.62, 0.91, 1.1], [1.43, 0.55, 1.2], [0.81, 0.21, 1.15]])
        v = np.concatenate([sv] + [np.array(t) for t in tris.values()], 0)
        rows, kinds = [], []
        for k, kind in enumerate(tris):                # the extra faces spread between the sheet's: the sheet's ids shift
            rows += list(sf[12 * k:12 * (k + 1)]) + [[sv.shape[0] + 3 * k + j for j in range(3)]]
            kinds += ["sheet"] * 12 + [kind]
        f = np.array(rows)
        extra = dict(kinds=kinds, alone=[i for i, k in enumerate(kinds) if k in ("sheet", "crossing")])
        v = np.stack([v, v + np.array([-0.0171, 0.0233, 0.0])])
    elif name == "empty_frame":
        S = 72
        v0, f = grid(3, 3, 0.21, 0.64, -0.31, 0.27, z=1.4)
        v1, _ = grid(3, 3, 3.2, 3.6, -0.31, 0.27, z=1.4)
        v2, _ = grid(3, 3, -0.93, 0.91, -0.89, 0.93, z=1.4)
        v = np.stack([v0, v1, v2])
    elif name in ("moves_a", "moves_b"):
        S = 96
        lo, hi = (0.05, 0.85) if name == "moves_a" else (-0.93, -0.45)
        v0, f = grid(4, 4, lo, hi, lo + 0.013, hi - 0.017, z=1.3)
        v = np.stack([v0, v0 + np.array([0.0113, -0.0091, 0.1])])
    elif name == "order":
        S, B = 512, 130
        f = np.array([[0, 1, 2], [0, 2, 3]])
        b = np.arange(B)
        st = (b * 37) % 64
        cx = (st % 8) * 64 + 20 + (b % 7) * 3.3
        cy = (st // 8) * 64 + 25 + (b % 5) * 4.1
        quad = np.array([[-3.1, -2.7], [3.3, -2.9], [2.9, 3.2], [-2.8, 3.4]])
        px = cx[:, None] + quad[None, :, 0]
        py = cy[:, None] + quad[None, :, 1]
        v = np.stack([1.0 - (2.0 * px + 1.0) / S, 1.0 - (2.0 * py + 1.0) / S, 1.2 + 0.01 * b[:, None] + 0.05 * np.arange(4)[None]], -1)
        extra = dict(super_of_frame=st)
    else:
        raise KeyError(name)
    return dict(name=name, S=S, B=v.shape[0], ndc=torch.from_numpy(np.asarray(v)).float().contiguous(), faces=torch.from_numpy(f).long(),
                blur=R.f32(blur), sigma=R.f32(sigma), **extra)


def references(c, grad=True):
    """float64 hard and soft rasterisation of a case + the float32 evaluation of both"""
    hard = R.rasterize(c["ndc"], c["faces"], c["S"])
    soft = R.rasterize(c["ndc"], c["faces"], c["S"], c["blur"], c["sigma"], grad=grad)
    return hard, soft


def conditions(c, hard, soft):
    """the case forces its path: asserted on the reference's data.  Returns what it found (printed, recorded in docs/NOTEBOOK.md)."""
    name, S, B, F = c["name"], c["S"], c["B"], c["faces"].shape[0]
    n_cov = int(soft["pix"].numel())
    n_und = int(soft["undecided"].sum()) + int(soft["undecided_uncovered"].numel()) + int(hard["undecided"].sum())
    info = dict(covered=n_cov, undecided=n_und, rim=int(soft["rim_wide"].sum()), max_tile=int(soft["tile_count"].max()), max_super=int(soft["super_count"].max()),
                max_tile_hard=int(hard["tile_count"].max()), max_cand=int(soft["ncand"].max()), max_tile_pairs=int(R.tile_pairs(soft).max()))
    assert n_und <= 0.02 * n_cov, info                                   # move the vertices, not the cap
    # pixels with 1e-3 < alpha < 1 - 1e-3: a few hundred with the half-pixel band, the pixels of the chosen row with the workload's
    # (the fan lies inside one tile, 230 covered pixels in all: 50)
    assert info["rim"] >= (10 if name in WORKLOAD else 50 if name == "fan" else 200), info
    near = hard["face_id"][hard["face_id"] >= 0]
    if name.startswith("one_face"):
        assert S % R.SUPER != 0 and S % R.TILE != 0 and (soft["super_count"] > 0).all()          # all four super-tiles, ragged last tile and super-tile
        last = R.dense(hard, "face_id", -1)[:, (S // R.TILE) * R.TILE:, :]
        assert (last >= 0).any()
    if name == "one_face_w":
        a = R.dense(soft, "alpha", 0.0)[0, 20]
        info["rim_pixels_of_row_20"] = int(((a > 0.5) & (a < 0.95)).sum())
        assert info["rim_pixels_of_row_20"] >= 30, info
    if name.startswith("fan"):
        assert F >= 600 and info["max_tile"] > K_STAGE and info["max_tile_hard"] > K_STAGE, info          # several staging rounds, MODE 0 / 1 / 2
        assert name == "fan_w" or info["max_cand"] > 50, info                 # the product over ALL candidates differs from a K = 50 cap
        assert info["max_super"] > 2 * K_STAGE
    if name == "fan_w":
        a = R.dense(soft, "alpha", 0.0)[0, 24]
        info["rim_pixels_of_row_24"] = int(((a > 0.01) & (a < 0.99)).sum())
        assert info["rim_pixels_of_row_24"] >= 3, info
    if name == "many_faces":
        W64 = (F + 63) // 64
        assert F > 8192 and F % 64 != 0 and W64 > 128
        info.update(nearest_ids_from_8192=int((near >= 8192).sum()), nearest_ids_in_the_last_word=int((near >= (W64 - 1) * 64).sum()),
                    nearest_ids_in_the_second_word_of_a_lane=int(((near >= 4096) & (near < 8192)).sum()))
        assert info["nearest_ids_from_8192"] > 0 and info["nearest_ids_in_the_last_word"] > 0 and info["max_tile"] > K_STAGE, info
    if name == "layers":
        lo, hi = c["tie"]
        far, nr = c["close"]
        assert hi > lo and nr > far
        n_lo = int((near == lo).sum())
        info.update(pixels_of_the_tied_face=n_lo, pixels_of_the_near_face=int((near == nr).sum()), distinct_nearest_faces=int(torch.unique(near).numel()))
        assert n_lo >= 2 * B and not (near == hi).any() and (near == nr).sum() >= 4 * B and not (near == far).any(), info
        for k, (first, end) in enumerate(c["sheets"]):   # each of the three sheets is the nearest somewhere
            info[f"pixels_of_sheet_{k}"] = int(((near >= first) & (near < end)).sum())
            assert info[f"pixels_of_sheet_{k}"] >= 10 * B, info
    if name == "culled":
        kinds = np.array(c["kinds"])
        seen = np.unique(near.numpy())
        cand = np.unique(soft["pair_f"].numpy())
        for kind in ("behind", "near_vertex", "zero_area", "nan", "off_screen"):
            k = int(np.nonzero(kinds == kind)[0][0])
            assert k not in seen and k not in cand, kind
        for kind in ("behind", "near_vertex", "zero_area", "nan"):
            assert not soft["live"][:, int(np.nonzero(kinds == kind)[0][0])].any(), kind
        assert soft["live"][:, int(np.nonzero(kinds == "off_screen")[0][0])].all()
        k = int(np.nonzero(kinds == "crossing")[0][0])
        info["pixels_of_the_crossing_face"] = int((near == k).sum())
        assert info["pixels_of_the_crossing_face"] >= 4 and c["ndc"][:, c["faces"][k], 0].max() > 1.0
    if name == "empty_frame":
        nact = int((soft["super_count"] > 0).sum())
        info["nact"] = nact
        assert B == 3 and (soft["super_count"][1] == 0).all() and nact % 8 != 0 and (soft["super_count"][0] > 0).any(), info
        assert int((hard["super_count"] > 0).sum()) == nact
    if name.startswith("moves"):
        want = (0, 0) if name == "moves_a" else (1, 1)
        for ref in (hard, soft):
            occ = ref["super_count"] > 0
            assert occ[:, want[0], want[1]].all() and int(occ.sum()) == B, occ
    if name == "order":
        nst = ((S + 63) // 64) ** 2
        occ = hard["super_count"].reshape(B, nst) > 0
        assert B * nst > 8192 and (occ.sum(1) == 1).all() and (soft["super_count"].reshape(B, nst) > 0).sum() == B
        assert torch.equal(occ.float().argmax(1), torch.from_numpy(c["super_of_frame"]))
        info["nact"] = int(occ.sum())
    print(f"[{name}] conditions: {info}")
    return info
