"""No GPU: the NumPy paths of harp_amd.utils.eval_util's geometric evaluation (align_w_scale, align_by_trafo, EvalUtil) and the float64
restatement tests/_pose_eval_ref.py against what the reference project's utils/eval_util.py returned for the same inputs (tests/golden/
pose_eval_ref.npz, written by tests/golden/make_golden_pose_eval.py); the three C entry points refuse empty sizes before any launch.
Tolerance 1e-12 relative to the largest magnitude of the compared array: both sides are the same float64 arithmetic (the K = 3 and other
rank-deficient cases differ in no recorded quantity but R, whose third singular direction is free there: R is compared where the
reference's own sigma3 / sigma1 >= 1e-3)."""
import os

import numpy as np
import pytest

from tests import _pose_eval_ref as PR

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_eval_ref.npz"))
CASES = [str(c) for c in G["cases"]]


def close(got, want, rel=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= rel * max(np.abs(want).max(), 1.0), np.abs(got - want).max()


def test_fixture_holds_the_cases():
    assert CASES == ["k21_n05", "k21_n3", "k21_n8", "k21_mirror", "k4", "k3", "k778"]
    assert np.linalg.det(G["k21_mirror_R"]) < -0.999 and np.linalg.det(G["k21_n3_R"]) > 0.999
    assert G["k778_gt"].dtype == np.float32 and G["k778_gt"].shape == (778, 3) and G["pck_vis"][:, 13].sum() == 0


@pytest.mark.parametrize("name", CASES)
def test_align_w_scale_numpy_path(name):
    from harp_amd.utils.eval_util import align_by_trafo, align_w_scale
    gt, pred = G[name + "_gt"].astype(np.float64), G[name + "_pred"].astype(np.float64)
    close(align_w_scale(gt, pred), G[name + "_aligned"])
    R, s, s1, t = align_w_scale(gt, pred, return_trafo=True)
    close(R, G[name + "_R"]); close(s, G[name + "_s"]); close(s1, G[name + "_s1"]); close(t, G[name + "_t"])
    close(align_by_trafo(pred, (G[name + "_R"], float(G[name + "_s"]), float(G[name + "_s1"]), G[name + "_t"])), G[name + "_by_trafo"])


def test_align_by_trafo_tensor_path():
    import torch
    from harp_amd.utils.eval_util import align_by_trafo
    name = "k21_n3"
    tr = (G[name + "_R"], float(G[name + "_s"]), float(G[name + "_s1"]), G[name + "_t"])
    got = align_by_trafo(torch.from_numpy(G[name + "_pred"]), tr)
    close(got.numpy(), G[name + "_by_trafo"])
    got = align_by_trafo(torch.from_numpy(np.stack([G[name + "_pred"]] * 2)), [tr, tr])
    close(got[1].numpy(), G[name + "_by_trafo"])


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    r = PR.procrustes(G[name + "_gt"][None], G[name + "_pred"][None])
    close(r["aligned"][0], G[name + "_aligned"])
    close(r["err"][0], np.linalg.norm(G[name + "_gt"].astype(np.float64) - G[name + "_aligned"], axis=1))
    close(r["trafo"][0, 9:], np.concatenate([[G[name + "_s"], G[name + "_s1"]], G[name + "_t"]]))
    close(r["sigma"][0], G[name + "_sigma"], rel=1e-9)
    if name == "k3":
        assert r["sigma"][0, 2] / r["sigma"][0, 0] < 1e-12 and r["sigma"][0, 1] / r["sigma"][0, 0] >= 1e-3
    else:
        assert r["sigma"][0, 2] / r["sigma"][0, 0] >= 0.02
        close(r["trafo"][0, :9].reshape(3, 3), G[name + "_R"])


def test_eval_util_numpy_path():
    from harp_amd.utils.eval_util import EvalUtil
    ev, eb = EvalUtil(num_kp=21), EvalUtil(21)
    for i in range(7):
        ev.feed(G["pck_gt"][i].astype(np.float64), G["pck_vis"][i], G["pck_pred"][i].astype(np.float64))
    got = ev.get_measures(0, 50, 20)
    want = [G["pck_epe_mean"], G["pck_epe_median"], G["pck_auc"], G["pck_curve"], G["pck_thresholds"]]
    for g, w in zip(got, want):
        close(g, w)
    assert len(got) == 5 and got[3].shape == (20,)
    # the restatement used by the GPU tests, from the same table
    d = np.linalg.norm(G["pck_gt"].astype(np.float64) - G["pck_pred"].astype(np.float64), axis=2)
    for g, w in zip(PR.measures(d, G["pck_vis"] != 0, 0, 50, 20), want):
        close(g, w)
    # feed_batch on CPU tensors: float32 distances, host storage, the same curve
    import torch
    eb.feed_batch(torch.from_numpy(G["pck_gt"]), torch.from_numpy(G["pck_vis"]), torch.from_numpy(G["pck_pred"]))
    gb = eb.get_measures(0, 50, 20)
    assert np.array_equal(gb[3], G["pck_curve"])
    for g, w in zip(gb[:3], want[:3]):
        close(g, w, rel=1e-6)


def test_get_measures_needs_two_thresholds():
    from harp_amd.utils.eval_util import EvalUtil
    ev = EvalUtil(21)
    ev.feed(G["pck_gt"][0], G["pck_vis"][0], G["pck_pred"][0])
    for steps in (1, 0):
        with pytest.raises(ValueError):
            ev.get_measures(0, 50, steps)


def test_restated_fscore_and_counts_on_a_case_by_hand():
    gt = np.array([[[0, 0, 0], [10, 0, 0], [0, 10, 0]]], dtype=np.float32)
    pred = np.array([[[0, 0, 3], [10, 0, 6], [0, 30, 0], [0, 0, 3]]], dtype=np.float32)
    r = PR.fscore(gt, pred, np.array([5.0, 15.0], dtype=np.float32))
    assert np.array_equal(r["d2_gt"], [[9.0, 36.0, 109.0]]) and np.array_equal(r["d2_pred"], [[9.0, 36.0, 400.0, 9.0]])
    p, q = np.array([1 / 3, 1.0]), np.array([0.5, 0.75])
    assert np.allclose(r["out"][0], np.stack([p, q, 2 * p * q / (p + q)], -1), rtol=1e-15)
    assert np.array_equal(PR.fscore(gt, gt + 100.0, [5.0])["out"], [[[0.0, 0.0, 0.0]]])
    err = np.array([[1.0, np.nan], [2.0, 5.0], [np.nan, 7.0]], dtype=np.float32)
    c, n, s = PR.pck_counts(err, np.array([[1, 1], [1, 0], [1, 1]]), np.array([1.0, 2.0, 7.0], dtype=np.float32))
    assert np.array_equal(c, [[1, 2, 2], [0, 0, 1]]) and np.array_equal(n, [2, 1]) and np.array_equal(s, [3.0, 7.0])


@pytest.fixture(scope="module")
def lib():
    from harp_amd import build, _lib
    build.build(force=False, verbose=False)
    return _lib.lib()


def test_entry_points_refuse_empty_sizes_without_launch(lib):
    """only sizes are tried, with fake pointers that are never dereferenced: every refusal comes before the launch (include/harp_hip.h)"""
    f = 1 << 20
    for N, K, Kp in [(0, 21, 21), (-1, 21, 21), (2, 0, 0), (2, -1, -1), (2, 21, 0), (2, 21, -3)]:
        assert lib.harp_procrustes_align(f, f, f, f, N, K, Kp, f, f, f, f, None) == 1, (N, K, Kp)
    assert lib.harp_procrustes_align(f, f, None, f, 2, 21, 22, f, f, f, f, None) == 1           # Kp != K needs pred_idx
    for N, K, T in [(0, 21, 20), (-1, 21, 20), (4, 0, 20), (4, -2, 20), (4, 21, 0), (4, 21, -1)]:
        assert lib.harp_pck_counts(f, f, f, N, K, T, f, f, f, None) == 1, (N, K, T)
    for N, Kg, Kp, T in [(0, 5, 5, 2), (-1, 5, 5, 2), (1, 0, 5, 2), (1, 5, 0, 2), (1, -5, 5, 2), (1, 5, -5, 2), (1, 5, 5, 0), (1, 5, 5, -1),
                         (1, 5, 5, 513)]:
        assert lib.harp_point_set_fscore(f, f, f, N, Kg, Kp, T, f, f, f, None) == 1, (N, Kg, Kp, T)
    # NULL required pointers, valid sizes
    assert lib.harp_procrustes_align(None, f, None, None, 1, 3, 3, None, f, None, f, None) == 1
    assert lib.harp_procrustes_align(f, f, None, None, 1, 3, 3, None, None, None, f, None) == 1
    assert lib.harp_pck_counts(f, None, None, 1, 1, 1, f, f, f, None) == 1
    assert lib.harp_point_set_fscore(f, f, f, 1, 1, 1, 1, None, None, None, None) == 1


def test_jacobi_polar_factor_on_the_host(tmp_path):
    """the 3x3 one-sided Jacobi of csrc/pose_eval.hip (lane 0's work) compiled into a host program (its `main` calls the host instance; no GPU is touched) and compared with np.linalg.svd: R = U V^T
    and s = sum W to 1e-13 where sigma3 / sigma1 >= 1e-3; with a vanishing sigma3 (three points, coplanar sets) R stays orthogonal and acts
    like the reference's on everything M can see (R diag-free part: |(R - R_ref) V W| small); the zero matrix gives an orthogonal R and s = 0"""
    import subprocess
    from harp_amd.build import CSRC
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = tmp_path / "polar.cpp"
    src.write_text('#include "pose_eval.hip"\n#include <stdio.h>\nint main() { double M[9], R[9], s;\n'
                   ' while (scanf("%lf %lf %lf %lf %lf %lf %lf %lf %lf", M, M + 1, M + 2, M + 3, M + 4, M + 5, M + 6, M + 7, M + 8) == 9) {\n'
                   '  polar_no_det_fix(M, R, s); for (int i = 0; i < 9; ++i) printf("%.17g ", R[i]); printf("%.17g\\n", s); }\n return 0; }\n')
    exe = tmp_path / "polar"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-x", "hip", "-I", CSRC, "-I", os.path.join(CSRC, "..", "..", "include"),
                    str(src), "-o", str(exe)], check=True, capture_output=True)
    rng = np.random.default_rng(5)
    Ms = []
    for i in range(60):
        K = [3, 4, 21, 778][i % 4]
        a = rng.normal(size=(K, 3)) * np.array([40.0, 25.0, 15.0])
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        b = a @ q.T * (-1.0 if i % 5 == 0 else 1.0) + rng.normal(size=(K, 3)) * [0.01, 1.0, 10.0][i % 3]
        if i % 8 == 5:
            a[:, 2] = 0.0                                                  # a flat set: rank 2 whatever K
        a, b = a - a.mean(0), b - b.mean(0)
        Ms.append((a / np.linalg.norm(a)).T @ (b / np.linalg.norm(b)))
    Ms += [np.zeros((3, 3)), np.eye(3), np.diag([1.0, 1e-3, 1e-5]), np.outer([1.0, 2.0, 3.0], [0.5, 0.1, -1.0])]
    text = "\n".join(" ".join("%.17g" % x for x in M.ravel()) for M in Ms)
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(Ms)
    full = flat = 0
    for M, line in zip(Ms, out):
        v = np.array(line.split(), dtype=np.float64)
        R, s = v[:9].reshape(3, 3), v[9]
        U, W, Vt = np.linalg.svd(M)
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(s - W.sum()) <= 1e-14 * max(W[0], 1.0)
        if W[0] > 0 and W[2] / W[0] >= 1e-3:
            assert np.abs(R - U @ Vt).max() <= 1e-13
            full += 1
        else:
            assert np.abs((R - U @ Vt) @ (Vt.T * W)).max() <= 1e-14          # the same on the directions that carry weight
            flat += 1
    assert full >= 30 and flat >= 15
