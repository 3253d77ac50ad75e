"""Plain float64, differentiable torch reference of the kinematic-tree skinning layer (include/harp_hip.h: harp_tree_model,
harp_lbs_tree_fwd), written from the struct's contract alone, and the two synthetic trees of tests/test_gpu_arm_front_back.py: the
smallest models that reach what the production SMPL-X arm (NJ = 55, NB = 20, NV = 1026, center_joint = 21) cannot.

A model is a dict of float64 tensors v_template (NV,3), shapedirs (NV,3,NB), posedirs ((NJ-1)*9, NV*3), J_template (NJ,3), J_dirs (NJ,3,NB),
weights (NV,NJ), pose_mean (NJ,3) and of integer lists parents (parents[0] = -1, parents[j] < j), pose_src (NJ), joint_src (n_out), with
center_joint an int.  Anchored by tests/test_front_ref_cpu.py (against oracle.harp_ref.smplxarm_forward on the production model)."""
import functools

import numpy as np
import torch

from oracle import harp_ref as H

N_POSE_IN = 17


def tree_forward(model, in_pose, betas, transl):
    """in_pose (B,17,3), betas (B,NB), transl (B,3) -> verts_mm (B,NV,3), joints_mm (B,n_out,3)"""
    B, dt = in_pose.shape[0], in_pose.dtype
    par, src = model["parents"], model["pose_src"]
    NJ = len(par)
    zero = torch.zeros(B, 3, dtype=dt)
    aa = torch.stack([model["pose_mean"][j][None] + (in_pose[:, src[j]] if src[j] >= 0 else zero) for j in range(NJ)], 1)
    R = H.smplx_batch_rodrigues(aa.reshape(-1, 3)).view(B, NJ, 3, 3)
    pose_map = (R[:, 1:] - torch.eye(3, dtype=dt)).reshape(B, -1)
    vp = model["v_template"][None] + torch.einsum("vck,bk->bvc", model["shapedirs"], betas) + (pose_map @ model["posedirs"]).view(B, -1, 3)
    J = model["J_template"][None] + torch.einsum("jck,bk->bjc", model["J_dirs"], betas)
    GR, Gt = [R[:, 0]], [J[:, 0]]
    for j in range(1, NJ):
        p = par[j]
        GR.append(GR[p] @ R[:, j])
        Gt.append((GR[p] @ (J[:, j] - J[:, p])[..., None])[..., 0] + Gt[p])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)                      # (B,NJ,3,3), (B,NJ,3)
    At = Gt - (GR @ J[..., None])[..., 0]
    TR = torch.einsum("vj,bjrc->bvrc", model["weights"], GR)
    Tt = torch.einsum("vj,bjr->bvr", model["weights"], At)
    cj = model["center_joint"]
    centre = Gt[:, cj] if cj >= 0 else torch.zeros(B, 3, dtype=dt)
    shift = (transl - centre)[:, None]
    verts = ((TR @ vp[..., None])[..., 0] + Tt + shift) * 1000.0
    joints = torch.stack([(Gt[:, s] + shift[:, 0]) * 1000.0 if s >= 0 else verts[:, -s - 1] for s in model["joint_src"]], 1)
    return verts, joints


def arm_pose_src():
    """the joint each of the 17 in_pose rows drives on the SMPL-X arm: global orient, right wrist, the 15 joints of the right hand"""
    src = [-1] * 55
    src[0], src[21] = 0, 1
    for k in range(15):
        src[40 + k] = 2 + k
    return src


def host_from_arm(m):
    """the arrays of synth.make_smplx_arm_model as a host model (float32 / int numpy, the layout of `_host_model`)"""
    tips = np.asarray(m["tip_verts"], np.int64)
    return dict(name="arm", v_template=np.asarray(m["v_template"], np.float32), shapedirs=np.asarray(m["shapedirs"], np.float32),
                posedirs=np.asarray(m["posedirs"], np.float32), J_template=np.asarray(m["J_template"], np.float32),
                J_dirs=np.asarray(m["J_shapedirs"], np.float32), weights=np.asarray(m["weights"], np.float32),
                pose_mean=np.asarray(m["pose_mean"], np.float32).reshape(55, 3), parents=[-1] + [int(p) for p in m["parents"][1:]],
                pose_src=arm_pose_src(), joint_src=[j if j < 55 else -int(tips[j - 71]) - 1 for j in H.ARM_JOINT_IDX], center_joint=21)


def model64(host):
    """a host model's float32 values in float64, as tree_forward wants them"""
    out = {k: (torch.from_numpy(v).double() if isinstance(v, np.ndarray) else v) for k, v in host.items()}
    return out


def device_layout(host):
    """the arrays of a host model laid out as harp_amd.hand_models_harp.body_models.TreeDeviceModel lays them out (harp_tree_model's
    pointers, contiguous numpy float32 / int32) + weights_T (NJ,NV) of harp_arm_front and the struct's integers"""
    NV, NB = host["v_template"].shape[0], host["shapedirs"].shape[-1]
    NJ = host["J_template"].shape[0]
    c = np.ascontiguousarray
    i32 = lambda a: c(np.asarray(a, np.int32))
    pd = host["posedirs"]
    return dict(NV=NV, NJ=NJ, NB=NB, n_pose_in=N_POSE_IN, center_joint=host["center_joint"], n_joints_out=len(host["joint_src"]),
                v_template=c(host["v_template"]), shapedirs_T=c(host["shapedirs"].reshape(NV * 3, NB).T), posedirs_T=c(pd), posedirs=c(pd.T),
                J_template=c(host["J_template"]), J_dirs=c(host["J_dirs"].reshape(NJ * 3, NB)), weights=c(host["weights"]),
                pose_mean=c(host["pose_mean"].reshape(-1)), parents=i32(host["parents"]), pose_src=i32(host["pose_src"]),
                joint_src=i32(host["joint_src"]), weights_T=c(host["weights"].T))


def depth_of(parents):
    d = [0] * len(parents)
    for j in range(1, len(parents)):
        d[j] = d[parents[j]] + 1
    return d


def _dyadic_weights(NV, NJ, rng, fixed):
    """(NV,NJ) float32 rows of dyadic weights (exact zeros elsewhere, each row sums to 1 exactly); fixed: {vertex: {joint: weight}}"""
    w = np.zeros((NV, NJ), np.float32)
    parts = [0.5, 0.25, 0.125, 0.0625, 0.0625]
    for v in range(NV):
        if v in fixed:
            for j, x in fixed[v].items():
                w[v, j] = x
        else:
            w[v, rng.choice(NJ, len(parts), replace=False)] = parts
    assert (w.sum(1) == 1.0).all() and ((w == 0).sum(1) >= NJ - 5).all()
    return w


@functools.lru_cache(maxsize=None)
def build_tree(name):
    """host model (float32 / int numpy; never modified) of a synthetic tree on a base mesh of tests/test_gpu_mesh_chain.py:
      twig : mesh `five` (NV = 6), NJ = 29, NB = 10, center_joint = -1; joints 0..16 one path driven by rows 0..16, joints 17..28 undriven
             leaves along it; joint_src = [16, -4, -4, 28] (two output joints on vertex 3); vertex 5 wholly on joint 28, vertex 0 on 0, 27, 28
      crown: mesh `hub` (NV = 13), NJ = 64, NB = 32, center_joint = 63; a seeded tree, 17 seeded driven joints (0 and 63 among them);
             64 output joints: 40 chain joints and 24 vertex joints (every vertex at least once, eleven twice)
    Positions are hand-sized (tens of mm); pose_mean is non-zero on every joint, the undriven ones included."""
    from tests.test_gpu_mesh_chain import _mesh_tables
    twig = name == "twig"
    assert twig or name == "crown"
    rng = np.random.default_rng(29 if twig else 64)
    _, P0, _, _ = _mesh_tables("five" if twig else "hub")
    NV = P0.shape[0]
    NJ, NB = (29, 10) if twig else (64, 32)
    if twig:
        parents = [-1] + list(range(16)) + [i + 2 for i in range(12)]
        pose_src = list(range(17)) + [-1] * 12
        joint_src = [16, -4, -4, 28]
        center = -1
        fixed = {5: {28: 1.0}, 0: {0: 0.5, 27: 0.25, 28: 0.25}}
    else:
        parents = [-1] + [int(rng.integers(max(0, j - 9), j)) for j in range(1, NJ)]
        driven = sorted([0, 63] + [int(j) for j in rng.choice(np.arange(1, 63), 15, replace=False)])
        pose_src = [-1] * NJ
        for i, j in enumerate(driven):
            pose_src[j] = (i * 5) % N_POSE_IN                               # a permutation of the rows: 5 and 17 are coprime
        chain = sorted([0, 63] + [int(j) for j in rng.choice(np.arange(1, 63), 38, replace=False)])
        vert = list(range(NV)) + [int(v) for v in rng.choice(NV, 24 - NV, replace=False)]
        joint_src = chain + [-v - 1 for v in vert]
        joint_src = [joint_src[i] for i in rng.permutation(64)]
        center = 63
        fixed = {}
    n = lambda *s: rng.standard_normal(s)
    host = dict(name=name, v_template=(P0 * 1e-3).astype(np.float32), shapedirs=(n(NV, 3, NB) * 1e-3).astype(np.float32),
                posedirs=(n((NJ - 1) * 9, NV * 3) * 1e-3).astype(np.float32), J_template=(n(NJ, 3) * 0.03).astype(np.float32),
                J_dirs=(n(NJ, 3, NB) * 1e-3).astype(np.float32), weights=_dyadic_weights(NV, NJ, rng, fixed),
                pose_mean=(n(NJ, 3) * 0.2).astype(np.float32), parents=parents, pose_src=pose_src, joint_src=joint_src, center_joint=center)
    return host


def assert_tree_property(host):
    """what each synthetic tree is there for, asserted from its tables (kSkinBatch = 28, kChainParts = 4, kArmWide = 320, MAXJ = 64, MAXB = 32
    of csrc/arm_front.hip / lbs_tree_body.h)"""
    name, par, src, jsrc, w = host["name"], host["parents"], host["pose_src"], host["joint_src"], host["weights"]
    NV, NJ = w.shape
    NB = host["shapedirs"].shape[-1]
    K = (NJ - 1) * 9 + NB
    per = (NV + 3) // 4
    depth = depth_of(par)
    assert par[0] == -1 and all(par[j] < j for j in range(1, NJ)) and sorted(s for s in src if s >= 0) == list(range(N_POSE_IN))
    if name != "arm":                                                         # both synthetic trees: undriven joints rotate, weights have exact zeros
        undriven = [j for j in range(NJ) if src[j] < 0]
        assert undriven and (np.abs(host["pose_mean"][undriven]).min(1) > 0).all()
        assert (w.sum(1) == 1.0).all() and (w == 0).any(1).all()
    if name == "twig":
        assert (NV, NJ, NB, host["center_joint"]) == (6, 29, 10, -1) and max(depth) == 16 == depth[16] and src[:17] == list(range(17))
        assert jsrc == [16, -4, -4, 28]                                       # two output joints on vertex 3
        assert NJ - 28 == 1                                                   # the second kSkinBatch trip: one live row, 27 clamped reads
        assert per == 2 and 3 * per >= NV                                     # wide part 3 starts at v = 6: no vertex
        assert w[5, 28] == 1.0 and set(np.nonzero(w[0])[0]) == {0, 27, 28}
        assert 64 // NB == 6 and K == 262 and K % 4 == 2                      # nch = 6 in the shape tail
    elif name == "crown":
        assert (NV, NJ, NB, host["center_joint"]) == (13, 64, 32, 63) and src[0] >= 0 and src[63] >= 0
        assert len(jsrc) == 64 and sum(s >= 0 for s in jsrc) == 40 and len({s for s in jsrc if s >= 0}) == 40
        named = [-s - 1 for s in jsrc if s < 0]
        assert set(named) == set(range(NV)) and len(named) == 24 and max(named.count(v) for v in range(NV)) == 2
        assert (NJ + 27) // 28 == 3 and NJ - 56 == 8 and 64 // NB == 2        # three kSkinBatch trips (28 + 28 + 8); nch = 2
        assert 256 + len(jsrc) == 320 and 256 + NJ == 320                     # the wide kernels' lanes 256..319 used to the last one
    else:
        assert (NV, NJ, NB, host["center_joint"]) == (1026, 55, 20, 21) and max(depth) == 10 and len(jsrc) == 22
