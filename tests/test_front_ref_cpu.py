"""CPU: tests/_front_ref.py, the float64 composition the fused MANO front and back are held to (tests/test_gpu_step_front_back.py), is itself
checked: it is the three pinned pieces called one after another, its autograd agrees with central differences, and its gradient rows add up
over a repeated frame and over the shared light the way the table scatter of the fused back has to."""
import functools

import torch

from tests import _chain_ref as C
from tests import _front_ref as R

F64 = torch.float64
FID = torch.tensor([4, 4, 0, 6, 4])                        # one frame three times, rows 1, 2, 3, 5 absent


@functools.lru_cache(maxsize=None)
def _setup():
    from harp_amd import synth
    from tests.test_gpu_mesh_chain import _case, _cotangents
    model = synth.make_mano_model(seed=0)
    cs = _case("mano", 1)                                  # the MANO template's tables (host side only)
    B = FID.shape[0]
    cot = {k: v.double() for k, v in _cotangents(dict(cs, B=B, vertical=None)).items()}
    return dict(m64=R.mano_model(model), edges0=torch.from_numpy(cs["edges0_np"]).long(), faces=torch.from_numpy(cs["faces_np"]).long(),
                tb={k: v.double() for k, v in R.case_tables(model).items()}, disp=cs["disp"].double(), cot=cot,
                g_colors=torch.randn(9, generator=torch.Generator().manual_seed(5), dtype=F64))


def _front(s, tb, fid, disp, share_light=0, self_shadow=1):
    return R.front(tb, fid, disp, s["edges0"], s["faces"], s["m64"], share_light, self_shadow)


def _slot(cot, b):
    return {k: v[b:b + 1] for k, v in cot.items()}


def test_front_is_the_three_pieces_one_after_another_bit_for_bit():
    from oracle import harp_ref as H
    from tests.test_gpu_frame_glue import FOCAL, S, _definition
    s = _setup()
    for share_light, self_shadow in ((0, 1), (1, 0)):
        out = _front(s, s["tb"], FID, s["disp"], share_light, self_shadow)
        d = _definition(s["tb"], FID, False, share_light, self_shadow)
        v, j = H.mano_forward(s["m64"], d["pose48"], d["betas"], d["trans_b"])
        cam_R = torch.diag(torch.tensor([-1.0, -1.0, 1.0], dtype=F64)).repeat(FID.shape[0], 1, 1)
        ch = C.chain(v, j, cam_R, d["cam_T"], d["light_pos"], s["disp"], s["edges0"], s["faces"], S, FOCAL)
        want = dict(d, cam_R=cam_R, verts_mm=v, joints_mm=j, **ch)
        assert set(out) == set(want) == set(R.ROW_KEYS) | {"verts_mm", "joints_mm"} | set(C.FWD_KEYS)
        for k in want:
            assert out[k].dtype == F64 and torch.equal(out[k], want[k]), k
        # the geometry the GPU test's bounds assume: the hand in front of both cameras, (almost) no clamped normal
        assert out["ndc_c"][..., 2].min() > 0.3 and out["ndc_l"][..., 2].min() > 1.0
        assert (out["il1"] == 0).sum() <= 3 and (out["il2"] == 0).sum() <= 3


def test_table_gradients_agree_with_central_differences():
    """Four entries per table (three of rows in FID, chosen by a seeded generator, and one of an absent row, whose gradient and difference
    quotient are both exactly 0) and four of disp, central differences in float64.

    Measured conditioning (this scene, |f| = 1.46): the error of the quotient falls as h^2 down to h = 1e-5 for the tables (worst
    3.2 h^2: a finger joint at angle 1e-5) and, for disp, whose length scale is the 1 mm displacement, as 4e4 h^2 down to h = 1e-7; below
    that the rounding of f takes over (<= 5e-16 / h).  So h = 1e-5 for the tables (truncation <= 3.2e-10, rounding <= 5e-11) and
    h = 1e-7 for disp (4e-10 and 5e-9), and the tolerance is ten times the sum: 4e-9 and 5e-8, absolute; the gradients compared lie
    between 2e-3 and 1 (one finger entry at 2e-9, which the absolute bound covers)."""
    s = _setup()
    f = lambda tb, disp: R.total(_front(s, tb, FID, disp), s["cot"], s["g_colors"])
    g = R.table_grads(s["tb"], s["disp"], f)
    gen = torch.Generator().manual_seed(7)
    pick = lambda n: int(torch.randint(0, n, (1,), generator=gen))
    worst = {}
    for k in R.TABLE_KEYS + ("disp",):
        src = s["disp"] if k == "disp" else s["tb"][k]
        h, tol = (1e-7, 5e-8) if k == "disp" else (1e-5, 4e-9)
        entries = [(r, pick(src.shape[1])) for r in (4, 0, 6, 2)] if src.dim() == 2 else sorted({(pick(src.numel()),) for _ in range(4)})
        for idx in entries:
            vals = []
            for sign in (1.0, -1.0):
                tb, disp = {kk: v.clone() for kk, v in s["tb"].items()}, s["disp"].clone()
                (disp if k == "disp" else tb[k])[idx] += sign * h
                with torch.no_grad():
                    vals.append(f(tb, disp).item())
            fd, an = (vals[0] - vals[1]) / (2 * h), g["g_" + k][idx].item()
            worst[k] = max(worst.get(k, 0.0), abs(fd - an) / tol)
            if src.dim() == 2 and idx[0] == 2:
                assert fd == 0.0 and an == 0.0, (k, idx)                   # a row no frame names
            else:
                assert an != 0.0 and abs(fd - an) <= tol, (k, idx, fd, an)
    print("[front_ref central differences] worst |fd - autograd| / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_a_repeated_frame_gets_the_sum_of_its_slots_and_the_shared_light_everything():
    s = _setup()
    B = FID.shape[0]
    per_row = ("g_pose", "g_rot", "g_trans", "g_cam", "g_light_positions")
    for share_light in (0, 1):
        g = R.table_grads(s["tb"], s["disp"], lambda tb, disp: R.total(_front(s, tb, FID, disp, share_light), s["cot"], s["g_colors"]))
        slots = [R.table_grads(s["tb"], s["disp"], lambda tb, disp, b=b: R.total(_front(s, tb, FID[b:b + 1], disp, share_light), _slot(s["cot"], b)))
                 for b in range(B)]
        for k in per_row:
            for r in range(7):
                if k == "g_light_positions" and share_light:
                    want = sum(sl[k][0] for sl in slots) if r == 0 else torch.zeros(3, dtype=F64)      # row 0 takes the whole sum
                else:
                    want = sum((sl[k][r] for b, sl in enumerate(slots) if int(FID[b]) == r), torch.zeros_like(g[k][r]))
                assert torch.allclose(g[k][r], want, rtol=1e-12, atol=1e-15), (share_light, k, r)
                assert (want.abs().max() > 0) == (r in (0, 4, 6) if not (k == "g_light_positions" and share_light) else r == 0), (k, r)
        # row 4 is three slots: no single slot explains it
        assert all((g["g_pose"][4] - sl["g_pose"][4]).abs().max() > 1e-6 for sl in slots)
        # the tables without rows sum over every slot (the slots' terms of an element may cancel: absolute, on the table's scale)
        for k in ("g_shape", "g_disp"):
            assert torch.allclose(g[k], sum(sl[k] for sl in slots), rtol=0, atol=1e-12 * g[k].abs().max().item()), k
