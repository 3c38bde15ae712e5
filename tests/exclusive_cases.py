"""What the exclusive-class tests share: inputs with the awkward cells in them, and host restatements of the
definitions in include/lss_convs.h / include/lss_simbev.h (ABI 34) -- the softmax cross-entropy and its gradient in
any float type, the argmax rule, the confusion counts and the paint-order class map."""
import numpy as np
import torch

TINY = float(np.finfo(np.float32).tiny)
LOSS_RTOL, LOSS_ATOL = 2e-6, 1e-7  # the project's bars for a loss (tests/test_gpu_focal_loss.py)
# (B, C, H, W): scalar arm (plane 25), scalar arm (plane 9), vector arm, vector arm with a sample spanning two
# blocks (257 threads), one thread per sample
SHAPES = [(2, 3, 5, 5), (1, 2, 1, 9), (4, 8, 16, 16), (3, 5, 1, 2056), (2, 4, 1, 8)]
VECTOR = {(4, 8, 16, 16), (3, 5, 1, 2056), (2, 4, 1, 8)}


def weights(C):
    """Non-uniform class weights; from three classes on, one of them is 0."""
    return torch.tensor([0.5, 2.0, 0.0, 1.25, 3.0, 0.75, 1.5, 1.0][:C], dtype=torch.float32)


def data(shape, dtype, seed=0):
    """(logits, labels): logits with a +60, a -60, a row of equal values and an exact tie of the two largest; labels
    with 255 and with values in C..254, which are ignored too."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    cells = (torch.randn(B * H * W, C, generator=g) * 3.0)
    n = cells.shape[0]
    cells[0] = 0.25
    cells[1 % n, 0] = 60.0
    cells[2 % n, C - 1] = -60.0
    cells[3 % n] = cells[3 % n, 0].item()
    cells[4 % n] = -1.0
    cells[4 % n, :2] = 1.5
    x = cells.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous().to(dtype)
    labels = torch.randint(0, C, (B, H, W), generator=g).to(torch.uint8)
    r = torch.rand(B, H, W, generator=g)
    labels[r < 0.1] = 255
    labels[(r >= 0.1) & (r < 0.15)] = C
    labels[(r >= 0.15) & (r < 0.2)] = 254
    flat = labels.view(-1)
    flat[5 % n], flat[6 % n], flat[7 % n] = 255, C, 254
    flat[0], flat[1 % n], flat[2 % n] = 0, 0, C - 1
    return x, labels


def mask(shape, seed=0, p=0.6):
    g = torch.Generator().manual_seed(1000 + seed)
    v = (torch.rand(shape[0], *shape[2:], generator=g) < p).to(torch.uint8)
    v.view(-1)[0], v.view(-1)[-1] = 1, 0
    return v


def counted(labels, valid, C):
    on = labels < C
    return on if valid is None else on & (valid != 0)


def closed_form(x, labels, valid, w):
    """(loss, d loss / dx) in x's float type (float64: the reference; float32: the formula's own rounding):
    l = w_y (m + log S - x_y), dl/dx_c = w_y (p_c - [c = y]) over the counted cells, both over max(W, tiny). The
    c = y element is evaluated as -w_y (sum of the other e_c) / S, the same number without the cancellation (in
    float64 too: 1 - p_y reaches 1e-9 here, which p_y - 1 would hold to seven digits only)."""
    C = x.shape[1]
    on = counted(labels, valid, C)
    y = torch.where(on, labels, torch.zeros_like(labels)).long()
    xs = torch.where(on.unsqueeze(1), x, torch.zeros_like(x))  # cells that do not count: selected out
    w = w.to(x.dtype)
    m = xs.max(dim=1, keepdim=True).values
    e = torch.exp(xs - m)
    S = e.sum(dim=1, keepdim=True)
    hot = torch.nn.functional.one_hot(y, C).movedim(-1, 1).bool()
    wy = w[y]
    xy = xs.gather(1, y.unsqueeze(1)).squeeze(1)
    l = wy * ((m.squeeze(1) - xy) + torch.log(S.squeeze(1)))
    others = torch.where(hot, torch.zeros_like(e), e).sum(dim=1, keepdim=True)
    g = wy.unsqueeze(1) * torch.where(hot, -(others / S), e / S)
    onf = on.to(x.dtype)
    W = (wy * onf).sum()
    if W.item() <= 0:
        return torch.zeros((), dtype=x.dtype), torch.zeros_like(x)
    d = W.clamp(min=TINY)
    return (l * onf).sum() / d, g * onf.unsqueeze(1) / d


def formula_rounding(x, labels, valid, w):
    """r32: the largest relative error, over gradient elements above 1e-12, of a float32 evaluation of closed_form
    against the float64 one on the same inputs."""
    _, g64 = closed_form(x.double(), labels, valid, w)
    _, g32 = closed_form(x.float(), labels, valid, w)
    big = g64.abs() > 1e-12
    if not big.any():
        return 0.0
    return ((g32.double() - g64).abs()[big] / g64.abs()[big]).max().item()


def rel_err(got, want):
    big = want.abs() > 1e-12
    return ((got - want).abs()[big] / want.abs()[big]).max().item() if big.any() else 0.0


def argmax_rule(x):
    """pred = argmax over the classes of (N, C, ...) float32 values with a strict > scanning upwards against a
    running best that starts at -inf: ties to the lowest class, a NaN never wins, all-NaN gives 0."""
    a = np.asarray(x, dtype=np.float32)
    best = np.zeros((a.shape[0],) + a.shape[2:], dtype=np.uint8)
    bv = np.full(best.shape, -np.inf, dtype=np.float32)
    for c in range(a.shape[1]):
        with np.errstate(invalid="ignore"):
            gt = a[:, c] > bv
        best = np.where(gt, np.uint8(c), best)
        bv = np.where(gt, a[:, c], bv)
    return best


def confusion_counts(x, labels, valid, nv):
    """conf[y][pred] as int64 over the counted cells of the first nv samples."""
    C = x.shape[1]
    pred = argmax_rule(x.float().numpy())[:nv]
    lab = labels.numpy()[:nv]
    on = counted(labels, valid, C).numpy()[:nv]
    conf = np.zeros((C, C), dtype=np.int64)
    np.add.at(conf, (lab[on].astype(np.int64), pred[on].astype(np.int64)), 1)
    return conf


def paint(masks):
    """The class map of (n, K, X, Y) group planes: 0 where none is set, else 1 + the highest set plane."""
    m = np.asarray(masks) != 0
    out = np.zeros((m.shape[0],) + m.shape[2:], dtype=np.uint8)
    for k in range(m.shape[1]):
        out = np.where(m[:, k], np.uint8(k + 1), out)
    return out


def class_index_ref(bev, groups):
    """lss_simbev_class_index without a warp, from the BEV channels: flipud, then the groups painted in order."""
    b = np.asarray(bev) > 0
    planes = np.stack([np.any(b[:, list(g)], axis=1)[:, ::-1, :] for g in groups], axis=1)
    return paint(planes)
