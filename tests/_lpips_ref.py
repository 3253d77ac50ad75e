"""Float64 CPU restatement of LPIPS v0.1 with net='alex' (lpips=True, spatial=False, eval mode), written from its definition with
torch.nn.functional: the scaling layer ((x - shift) / scale with the package's float32 constants), torchvision alexnet.features[0:12] with
taps after the five ReLUs, per-tap channel normalisation f / (||f||_2 + 1e-10), the non-negative lin weights on the squared difference,
the spatial mean, and the sum over the taps.  Weights in harp_amd.lpips' state-dict layout (b)."""
import torch
import torch.nn.functional as F

SHIFT = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float32).double()
SCALE = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float32).double()
CONV_KEYS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")


def features(x, sd):
    """x (N,3,H,W) float64 in LPIPS' input domain -> the five tap maps"""
    x = (x - SHIFT.view(1, 3, 1, 1)) / SCALE.view(1, 3, 1, 1)
    w = [(sd[k + ".weight"].detach().cpu().double(), sd[k + ".bias"].detach().cpu().double()) for k in CONV_KEYS]
    taps = []
    h = F.relu(F.conv2d(x, *w[0], stride=4, padding=2))
    taps.append(h)
    h = F.relu(F.conv2d(F.max_pool2d(h, 3, 2), *w[1], padding=2))
    taps.append(h)
    h = F.relu(F.conv2d(F.max_pool2d(h, 3, 2), *w[2], padding=1))
    taps.append(h)
    h = F.relu(F.conv2d(h, *w[3], padding=1))
    taps.append(h)
    h = F.relu(F.conv2d(h, *w[4], padding=1))
    taps.append(h)
    return taps


def lpips(X, Y, sd, normalize=False):
    """X, Y (N,3,H,W) -> {"total": (N,), "taps": (N,5)} in float64"""
    X, Y = X.double(), Y.double()
    if normalize:
        X, Y = 2 * X - 1, 2 * Y - 1
    fx, fy = features(X, sd), features(Y, sd)
    taps = []
    for k, (a, b) in enumerate(zip(fx, fy)):
        a = a / (a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        b = b / (b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        w = sd[f"lin{k}.model.1.weight"].detach().cpu().double().view(1, -1, 1, 1)
        taps.append(((a - b) ** 2 * w).sum(1).mean((1, 2)))
    taps = torch.stack(taps, 1)
    return {"total": taps.sum(1), "taps": taps}
