"""What the focal-loss tests share: the closed form of the loss written out independently of the package (in
whatever dtype the logits come in: fp64 for the reference, fp32 for the formula's own rounding), the naive form
autograd differentiates, the data and the per-class rows."""
import torch

GAMMAS = [0.0, 0.5, 2.0, 3.7]
LOSS_RTOL, LOSS_ATOL = 2e-6, 1e-7  # the project's bars for this loss (tests/test_gpu_loss.py)


def softplus(z):
    return torch.log1p(torch.exp(-z.abs())) + z.clamp(min=0)


def closed_form(x, t, rows):
    """(mean loss, d mean loss / dx) from the definition, in x's dtype. rows: K x 3 (w_pos, w_neg, gamma) for
    x (N, K, H, W)."""
    r = torch.as_tensor(rows, dtype=x.dtype).view(-1, 1, 1, 3)
    wp, wn, g = r[..., 0], r[..., 1], r[..., 2]
    q = t != 0
    p, pm = torch.sigmoid(x), torch.sigmoid(-x)
    l1 = torch.exp(-g * softplus(x)) * wp * softplus(-x)
    g1 = -torch.exp(-g * softplus(x)) * wp * (g * p * softplus(-x) + pm)
    l0 = torch.exp(-g * softplus(-x)) * wn * softplus(x)
    g0 = torch.exp(-g * softplus(-x)) * wn * (g * pm * softplus(x) + p)
    return torch.where(q, l1, l0).mean(), torch.where(q, g1, g0) / x.numel()


def naive(x, t, rows, subtract=True):
    """mean of (1 - p_t) ** gamma * weighted BCE, for autograd. subtract: 1 - p_t by subtraction, the form a user
    writes -- exactly 0 at a saturated, correct element (pow's backward is then inf * 0) and, short of that, off by
    eps / (1 - p_t) relative (5e-8 at |x| = 20 in fp64). Otherwise 1 - p_t = sigmoid(-z), which autograd
    differentiates to full precision: the reference for the agreement away from saturation."""
    r = torch.as_tensor(rows, dtype=x.dtype).view(-1, 1, 1, 3)
    wp, wn, g = r[..., 0], r[..., 1], r[..., 2]
    q = (t != 0).to(x.dtype)
    p = torch.sigmoid(x)
    one_minus = 1 - (q * p + (1 - q) * (1 - p)) if subtract else torch.sigmoid(torch.where(t != 0, -x, x))
    w = q * wp + (1 - q) * wn
    # -log(p_t); (binary_cross_entropy_with_logits adds and subtracts |x|: 1e-7 relative where the loss is tiny)
    bce = torch.nn.functional.softplus(torch.where(t != 0, -x, x))
    return (one_minus ** g * w * bce).mean()


def rows(K, gamma):
    """Distinct rows per class; class 0 keeps `gamma`, so gamma = 0 is tested as exactly 0."""
    return [(0.5 + 0.75 * k, 1.0 - 0.1 * k, gamma * (1.0 + 0.25 * k)) for k in range(K)]


def data(shape, dtype, seed=0):
    """Logits with +-60 and 0 among them and labels such that (60, 1), (-60, 0) (saturated and right), (60, 0),
    (-60, 1) (saturated and wrong) and 0 all occur."""
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.randn(shape, generator=g) * 4).to(dtype)
    t = (torch.rand(shape, generator=g) < 0.3).float()
    xs = torch.tensor([60.0, -60.0, 60.0, -60.0, 0.0])
    ts = torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0])
    n = min(5, x.numel())
    x.view(-1)[:n] = xs[:n].to(dtype)
    t.view(-1)[:n] = ts[:n]
    return x, t


def formula_rounding(x, t, r):
    """r32: the largest relative error, over gradient elements above 1e-12, of an fp32 evaluation of the closed
    form against the fp64 one on the same inputs -- the formula's own rounding."""
    _, g64 = closed_form(x.double(), t.double(), r)
    _, g32 = closed_form(x.float(), t.float(), r)
    big = g64.abs() > 1e-12
    if not big.any():
        return 0.0
    return ((g32.double() - g64).abs()[big] / g64.abs()[big]).max().item()
