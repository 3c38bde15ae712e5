"""lss_seg_loss_masked (tools.SimpleLoss / FocalLoss with valid=) and lss_seg_metrics_accum_masked
(tools.seg_metrics_accumulate with valid=) on the MI355X.

Loss shapes: (3, 3, 5, 7) -- 315 elements: one block with a tail vector, plane 35: a thread's 8 elements cross class
planes and samples, and the mask is read a byte at a time -- and (2, 3, 20, 20): two blocks, plane 400: the mask is
read 8 bytes at a time -- and (2, 3, 19, 21): two blocks with a ragged last vector (2394 elements), plane 399: threads
cross class planes beyond the first block and the mask index steps back mid-thread. fp32 and bf16 logits; rows: gamma 0 (BCE with pw 2.13), gamma 2 with alpha rows, gamma 0.5.
Reference: the fp64 restatement of tests/valid_mask_cases.py. Bars: those tests/test_gpu_focal_loss.py holds the
unmasked kernel to against the same closed form -- loss rtol 2e-6 / atol 1e-7; fp32 gradient rtol max(1e-5, 4 r32),
atol 1e-12; bf16 gradient 8e-3. Each case prints its measured errors."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import focal_cases as C  # noqa: E402
import valid_mask_cases as V  # noqa: E402
from lss_carla_amd import _lib, tools as T  # noqa: E402
from lss_carla_amd.predict import threshold_logit  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(3, 3, 5, 7), (2, 3, 20, 20), (2, 3, 19, 21)]
DTYPES = [torch.float32, torch.bfloat16]
ROWS = {"bce": [(2.13, 1.0, 0.0)] * 3, "focal2": [(0.25, 0.75, 2.0), (0.5, 0.5, 2.0), (0.75, 0.25, 2.0)],
        "focal05": C.rows(3, 0.5)}


def _mask(shape, seed=0, p=0.6):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape[0], *shape[2:], generator=g) < p).to(torch.uint8)


def _module(rows):
    fn = T.FocalLoss(len(rows)).to(DEV)
    fn.focal_params.copy_(torch.tensor(rows))
    return fn, fn.focal_params.cpu().tolist()


def _run(fn, x, t, valid=None, scale=0.75):
    xd = x.to(DEV).requires_grad_(True)
    loss = fn(xd, t.to(DEV)) if valid is None else fn(xd, t.to(DEV), valid.to(DEV))
    loss.backward(torch.tensor(scale, device=DEV))
    return loss.detach(), xd.grad


def _grad_tol(x, t, rows, dtype):
    if dtype == torch.bfloat16:
        return 8e-3
    return max(1e-5, 4 * C.formula_rounding(x, t, rows))


def _rel_err(got, want):
    big = want.abs() > 1e-12
    return ((got - want).abs()[big] / want.abs()[big]).max().item() if big.any() else 0.0


@pytest.fixture
def launched(monkeypatch):
    calls = []
    real = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real(code, what))[1])
    return calls


@pytest.mark.parametrize("kind", list(ROWS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_masked_loss_vs_fp64_restatement(shape, dtype, kind, launched):
    x, t = C.data(shape, dtype, seed=1)
    valid = _mask(shape)
    assert 0 < valid.sum() < valid.numel()
    fn, rows = _module(ROWS[kind])
    loss, grad = _run(fn, x, t, valid)
    assert launched == ["lss_seg_loss_masked", "lss_seg_loss_masked_bwd"]
    assert grad.dtype == dtype and loss.dtype == torch.float32 and loss.shape == ()
    want, wgrad = V.masked_closed_form(x.double(), t.double(), valid, rows)
    wgrad = 0.75 * wgrad
    tol = _grad_tol(x, t, rows, dtype)
    print(f"{shape} {dtype} {kind}: loss {loss.item():.9e} fp64 {want.item():.9e} rel "
          f"{abs(loss.item() - want.item()) / abs(want.item()):.2e}; grad rel err "
          f"{_rel_err(grad.cpu().double(), wgrad):.2e} (bar {tol:.2e})")
    torch.testing.assert_close(loss.cpu().double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(grad.cpu().double(), wgrad, rtol=tol, atol=1e-12)
    off = (valid == 0).unsqueeze(1).expand(shape)
    assert (grad.cpu()[off] == 0).all() and (grad.cpu()[~off] != 0).any()  # exactly 0 at masked cells
    loss2, grad2 = _run(fn, x, t, valid)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)  # two runs: equal bits
    if kind == "bce":  # SimpleLoss takes the same kernel with its weight as the rows (pw, 1, 0)
        ls, gs = _run(T.SimpleLoss(2.13).to(DEV), x, t, valid)
        lp, gp = _run(T.SimpleLoss([2.13] * 3).to(DEV), x, t, valid)
        assert torch.equal(ls, loss) and torch.equal(gs, grad) and torch.equal(lp, loss) and torch.equal(gp, grad)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_zero_mask_and_non_finite_logits_under_masked_cells(shape, dtype):
    x, t = C.data(shape, dtype, seed=2)
    fn, _ = _module(ROWS["focal05"])
    zero = torch.zeros(shape[0], *shape[2:], dtype=torch.uint8)
    lz, gz = _run(fn, x, t, zero)
    assert lz.item() == 0.0 and (gz == 0).all()
    valid = _mask(shape, seed=3)
    la, ga = _run(fn, x, t, valid)
    off = (valid == 0).unsqueeze(1).expand(shape)
    bad = x.clone()
    k = int(off.sum())
    bad[off] = torch.tensor([float("nan"), float("inf"), -float("inf")]).repeat(k // 3 + 1)[:k].to(dtype)
    lb, gb = _run(fn, bad, t, valid)
    assert torch.isfinite(lb) and torch.equal(la, lb) and torch.equal(ga, gb) and (gb.cpu()[off] == 0).all()
    # every logit NaN under the all-zero mask
    ln, gn = _run(fn, torch.full(shape, float("nan"), dtype=dtype), t, zero)
    assert ln.item() == 0.0 and (gn == 0).all()


@pytest.mark.parametrize("kind", list(ROWS))
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_ones_mask_is_the_unmasked_kernel(shape, dtype, kind):
    x, t = C.data(shape, dtype, seed=4)
    fn, rows = _module(ROWS[kind])
    ones = torch.ones(shape[0], *shape[2:], dtype=torch.uint8)
    lm, gm = _run(fn, x, t, ones)
    lu, gu = _run(fn, x, t)
    tol = _grad_tol(x, t, rows, dtype)
    print(f"{shape} {dtype} {kind}: loss rel {abs(lm.item() - lu.item()) / abs(lu.item()):.2e}, grad rel "
          f"{_rel_err(gm.double().cpu(), gu.double().cpu()):.2e} (bar {tol:.2e})")
    torch.testing.assert_close(lm, lu, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(gm.double(), gu.double(), rtol=tol, atol=1e-12)
    # the gradient is stored as the unmasked kernel stores it and the backward's extra factor n / M is exactly 1
    assert torch.equal(gm, gu)


def test_replay_follows_the_mask():
    shape = (3, 3, 5, 7)
    x, t = C.data(shape, torch.float32, seed=5)
    fn, _ = _module(ROWS["focal2"])
    m1, m2 = _mask(shape, seed=6), _mask(shape, seed=7, p=0.3)
    assert not torch.equal(m1, m2)
    a, ga = _run(fn, x, t, m1)
    b, gb = _run(fn, x, t, m2)
    assert not torch.equal(a, b)
    xd, td, vd = x.to(DEV).requires_grad_(True), t.to(DEV), m1.to(DEV).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        torch.autograd.grad(fn(xd, td, vd), xd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = fn(xd, td, vd)
        (grad,) = torch.autograd.grad(loss, xd, torch.full((), 0.75, device=DEV))
    graph.replay()
    assert torch.equal(loss, a) and torch.equal(grad, ga)
    vd.copy_(m2.to(DEV))  # in place: the replay reads the same address
    graph.replay()
    assert torch.equal(loss, b) and torch.equal(grad, gb)
    vd.zero_()
    graph.replay()
    assert loss.item() == 0.0 and (grad == 0).all()


def test_strided_misaligned_or_non_uint8_take_the_torch_path(launched):
    fn, rows = _module(ROWS["focal2"])
    shape = (2, 3, 5, 5)
    x, t = C.data(shape, torch.float32, seed=8)
    valid = _mask(shape, seed=9)
    buf = torch.zeros(x.numel() + 1, device=DEV)
    xm = buf[1:].view(shape)
    xm.copy_(x)
    xm.requires_grad_(True)
    assert xm.data_ptr() % 16 == 4
    got = fn(xm, t.to(DEV), valid.to(DEV))
    (g,) = torch.autograd.grad(got, xm)
    got_b = fn(x.to(DEV), t.to(DEV), valid.to(DEV).bool())  # a boolean mask: same values, the torch path
    assert not launched
    want, wgrad = V.masked_closed_form(x.double(), t.double(), valid, rows)
    torch.testing.assert_close(got.detach().cpu().double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(got_b.cpu().double(), want, rtol=C.LOSS_RTOL, atol=C.LOSS_ATOL)
    torch.testing.assert_close(g.cpu().double(), wgrad, rtol=_grad_tol(x, t, rows, torch.float32), atol=1e-12)
    with pytest.raises(RuntimeError):
        fn(x.to(DEV), t.to(DEV), valid.to(DEV)[:1])


def test_loss_entries_refuse_bad_arguments():
    lib = _lib.load()
    B, K, plane = 2, 2, 16
    n = B * K * plane
    x, t, grad = (torch.zeros(n + 8, device=DEV) for _ in range(3))
    valid = torch.ones(B * plane, device=DEV, dtype=torch.uint8)
    params = torch.ones(K, 3, device=DEV)
    partial = torch.zeros(2 * int(lib.lss_bce_partials(n)), device=DEV)
    loss, scale, gl = (torch.zeros(2, device=DEV) for _ in range(3))
    st = _lib.stream_handle(DEV)
    p = _lib.ptr

    def call(xp=p(x), tp=p(t), vp=p(valid), k=K, pp=p(params), gp=p(grad), pl=plane, count=n, lp=p(loss), ip=p(scale),
             dt=_lib.F32, part=p(partial)):
        return lib.lss_seg_loss_masked(xp, dt, tp, vp, count, pl, k, pp, part, lp, ip, gp, st)

    off = lambda v, by=2: ctypes.c_void_p(v.data_ptr() + by)  # noqa: E731
    assert call() == 0
    for bad in (dict(xp=None), dict(tp=None), dict(vp=None), dict(pp=None), dict(gp=None), dict(lp=None), dict(ip=None),
                dict(part=None), dict(k=0), dict(pl=0), dict(count=0), dict(count=n - 8), dict(pl=plane + 1), dict(dt=7),
                dict(xp=off(x)), dict(tp=off(t)), dict(gp=off(grad)), dict(pp=off(params)), dict(ip=off(scale))):
        assert call(**bad) == -1, bad  # LSS_CONV_EINVAL, before any launch

    def bwd(gp=p(grad), glp=p(gl), ip=p(scale), dp=p(x), count=n, dt=_lib.F32):
        return lib.lss_seg_loss_masked_bwd(gp, dt, count, glp, ip, dp, st)

    assert bwd() == 0
    for bad in (dict(gp=None), dict(glp=None), dict(ip=None), dict(dp=None), dict(count=0), dict(dt=7),
                dict(gp=off(grad)), dict(dp=off(x)), dict(ip=off(scale)), dict(glp=off(gl))):
        assert bwd(**bad) == -1, bad
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the masked metrics
def _metrics_ref(x, t, valid, rows, thetas, nv):
    """The totals of lss_seg_metrics_accum_masked restated in torch on the host: the fp32 logits the kernel sees, the
    loss term in fp64 (valid_mask_cases.masked_closed_form over the first nv samples), integer counts."""
    B, K = x.shape[:2]
    Tn = len(thetas)
    xs, ts, vs = x[:nv].float(), t[:nv], valid[:nv]
    on = (vs != 0).unsqueeze(1).expand_as(xs)
    out = [0.0] * (1 + K + 2 * K * Tn)
    if nv:
        mean, _ = V.masked_closed_form(xs.double(), ts.double(), vs, rows)
        out[0] = nv * mean.item()
    th = torch.tensor(thetas, dtype=torch.float32)
    for k in range(K):
        ok, q = on[:, k], ts[:, k] != 0
        out[1 + k] = int((ok & q).sum())
        for j in range(Tn):
            pp = ok & (xs[:, k] > th[j])
            out[1 + K + k * Tn + j] = int((pp & q).sum())
            out[1 + K + K * Tn + k * Tn + j] = int(pp.sum())
    return out, int((vs != 0).sum())


def _device_term_sum(x, t, valid, rows, nv):
    """The fp64 sum, over the valid elements of the first nv samples, of the device's own fp32 loss terms: per class,
    the valid elements compacted on the host into one sample of one class and summed by the unmasked entry
    (lss_seg_metrics_accum: totals[0] += sum / per_sample, an fp64 sum of the same focal_term)."""
    K = x.shape[1]
    th = torch.zeros(1, device=DEV)
    total = 0.0
    for k in range(K):
        on = valid[:nv] != 0
        xs, ts = x[:nv, k][on].contiguous(), t[:nv, k][on].contiguous()
        if xs.numel() == 0:
            continue
        tot = torch.zeros(4, device=DEV, dtype=torch.float64)
        T.seg_metrics_accumulate(xs.view(1, 1, 1, -1).to(DEV), ts.view(1, 1, 1, -1).to(DEV), tot, None,
                                 torch.tensor([rows[k]], device=DEV), th)
        total += tot[0].item() * xs.numel()
    return total


@pytest.mark.parametrize("nv", [None, 2, 0])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES + [(3, 1, 5, 7)])
def test_masked_metrics_vs_restatement(shape, dtype, nv, launched):
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=10)
    valid = _mask(shape, seed=11)
    rows = ROWS["focal05"][:K]
    ladder = [0.35, 0.5, 0.65]
    thetas = [threshold_logit(v) for v in ladder]
    params = torch.tensor(rows, device=DEV)
    th = torch.tensor(thetas, device=DEV, dtype=torch.float32)
    totals = torch.zeros(1 + K + 2 * K * 3, device=DEV, dtype=torch.float64)
    cells = torch.zeros(1, device=DEV, dtype=torch.float64)
    n_valid = None if nv is None else torch.tensor([nv], device=DEV, dtype=torch.int32)
    for _ in range(2):  # accumulates
        T.seg_metrics_accumulate(x.to(DEV), t.to(DEV), totals, n_valid, params, th, valid=valid.to(DEV), valid_cells=cells)
    assert launched == ["lss_seg_metrics_accum_masked"] * 2
    nvi = B if nv is None else nv
    want, m = _metrics_ref(x, t, valid, params.cpu().tolist(), th.cpu().tolist(), B if nv is None else nv)
    got = totals.cpu().tolist()
    assert got[1:] == [2.0 * v for v in want[1:]]                       # integer counts: exact
    assert cells.item() == 2.0 * m
    print(f"{shape} {dtype} nv {nv}: loss total {got[0]:.12e} want {2 * want[0]:.12e}")
    # the loss term: nv * S / max(M, 1) with S the fp64 sum of the per-element terms. Against the device's own fp32
    # terms summed in fp64 in another order: 1e-12 relative; against the fp64 closed form (whose terms differ from the
    # fp32 ones by the formula's rounding): the project's bar for this loss
    S = _device_term_sum(x, t, valid, params.cpu().tolist(), nvi)
    assert got[0] == pytest.approx(2 * nvi * S / max(m * K, 1), rel=1e-12, abs=0.0 if m else 1e-300)
    assert got[0] == pytest.approx(2 * want[0], rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
    # no valid_cells: the totals are the same
    again = torch.zeros_like(totals)
    T.seg_metrics_accumulate(x.to(DEV), t.to(DEV), again, n_valid, params, th, valid=valid.to(DEV))
    assert again.cpu().tolist() == [v / 2 for v in got]


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES)
def test_all_ones_mask_reproduces_the_unmasked_counts(shape, dtype):
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=13)
    params = torch.tensor(ROWS["bce"], device=DEV)
    th = torch.tensor([threshold_logit(v) for v in (0.4, 0.5, 0.6)], device=DEV, dtype=torch.float32)
    nv = torch.tensor([B - 1], device=DEV, dtype=torch.int32)
    ones = torch.ones(B, *shape[2:], device=DEV, dtype=torch.uint8)
    a = torch.zeros(1 + K + 2 * K * 3, device=DEV, dtype=torch.float64)
    b, cells = torch.zeros_like(a), torch.zeros(1, device=DEV, dtype=torch.float64)
    T.seg_metrics_accumulate(x.to(DEV), t.to(DEV), a, nv, params, th, valid=ones, valid_cells=cells)
    T.seg_metrics_accumulate(x.to(DEV), t.to(DEV), b, nv, params, th)
    a, b = a.cpu().tolist(), b.cpu().tolist()
    assert a[1:] == b[1:] and cells.item() == (B - 1) * shape[2] * shape[3]
    assert a[0] == pytest.approx(b[0], rel=1e-12)  # nv * S / M with M = nv K plane is S / (K plane)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_masked_metrics_of_misaligned_logits(dtype):
    """Logits that start one element into a larger buffer (contiguous, off every 16-byte boundary): the entry takes
    the guarded element loads for the whole call. Counts, cells and loss against the restatements above."""
    shape, ladder = (3, 3, 5, 5), [0.35, 0.5, 0.65]
    B, K = shape[:2]
    x, t = C.data(shape, dtype, seed=14)
    valid = _mask(shape, seed=15)
    buf = torch.zeros(x.numel() + 1, device=DEV, dtype=dtype)
    buf[1:] = x.to(DEV).view(-1)
    xm = buf[1:].view(shape)
    assert xm.is_contiguous() and xm.data_ptr() % 16 != 0
    params = torch.tensor(ROWS["focal05"], device=DEV)
    th = torch.tensor([threshold_logit(v) for v in ladder], device=DEV, dtype=torch.float32)
    for nv in (B, 2):
        totals = torch.zeros(1 + K + 2 * K * 3, device=DEV, dtype=torch.float64)
        cells = torch.zeros(1, device=DEV, dtype=torch.float64)
        n_valid = torch.tensor([nv], device=DEV, dtype=torch.int32)
        T.seg_metrics_accumulate(xm, t.to(DEV), totals, n_valid, params, th, valid=valid.to(DEV), valid_cells=cells)
        want, m = _metrics_ref(x, t, valid, params.cpu().tolist(), th.cpu().tolist(), nv)
        got = totals.cpu().tolist()
        assert got[1:] == [float(v) for v in want[1:]] and cells.item() == float(m)
        S = _device_term_sum(x, t, valid, params.cpu().tolist(), nv)
        print(f"{dtype} nv {nv}: loss total {got[0]:.12e} want {want[0]:.12e} device terms {nv * S / max(m * K, 1):.12e}")
        assert got[0] == pytest.approx(nv * S / max(m * K, 1), rel=1e-12)
        assert got[0] == pytest.approx(want[0], rel=C.LOSS_RTOL, abs=C.LOSS_ATOL)
        assert m > 0 and sum(want[1:]) > 0


def test_metrics_entry_refuses_bad_arguments():
    lib = _lib.load()
    B, K, plane, Tn = 2, 2, 16, 2
    per = K * plane
    x, t = torch.zeros(B * per, device=DEV), torch.zeros(B * per, device=DEV)
    valid = torch.ones(B * plane, device=DEV, dtype=torch.uint8)
    params, th = torch.ones(K, 3, device=DEV), torch.zeros(Tn, device=DEV)
    totals = torch.zeros(1 + K + 2 * K * Tn, device=DEV, dtype=torch.float64)
    cells = torch.zeros(2, device=DEV, dtype=torch.float64)
    nbytes = int(lib.lss_seg_metrics_masked_partial_bytes(x.numel(), K, Tn))
    assert nbytes == 8 + 4 * (2 * K * (Tn + 1) + 2)
    assert lib.lss_seg_metrics_masked_partial_bytes(x.numel(), K, 17) == 0
    assert lib.lss_seg_metrics_masked_partial_bytes(x.numel(), 33, 1) == 0
    partial = torch.zeros(nbytes // 8, device=DEV, dtype=torch.float64)
    st = _lib.stream_handle(DEV)
    p = _lib.ptr

    def call(xp=p(x), tp=p(t), vp=p(valid), pl=plane, k=K, rp=p(params), thp=p(th), tn=Tn, tot=p(totals), cp=p(cells),
             part=p(partial), batch=B, ps=per, dt=_lib.F32):
        return lib.lss_seg_metrics_accum_masked(xp, dt, tp, vp, ps, batch, None, pl, k, rp, thp, tn, tot, cp, part, st)

    off = lambda v, by=4: ctypes.c_void_p(v.data_ptr() + by)  # noqa: E731
    assert call() == 0 and call(cp=None) == 0
    for bad in (dict(xp=None), dict(tp=None), dict(vp=None), dict(rp=None), dict(thp=None), dict(tot=None),
                dict(part=None), dict(pl=0), dict(k=0), dict(k=33), dict(tn=0), dict(tn=17), dict(batch=0), dict(ps=per + 1),
                dict(dt=7), dict(tot=off(totals)), dict(cp=off(cells)), dict(part=off(partial)),
                dict(rp=off(params, 2)), dict(thp=off(th, 2))):
        assert call(**bad) == -1, bad
    torch.cuda.synchronize()
