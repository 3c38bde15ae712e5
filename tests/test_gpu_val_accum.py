"""lss_bce_iou_accum (tools.val_accumulate): a validation batch's loss x samples, intersection and union in
one pass, over the first n_valid samples, against a CPU fp64 reference
(binary_cross_entropy_with_logits(pos_weight, reduction="sum") / per_sample, exact counts). Loss at the
project's bar for this loss (tests/test_gpu_loss.py: rtol 2e-6, atol 1e-7); counts equal; two calls
accumulate; two runs are bit-equal; one captured graph follows n_valid rewritten between replays."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import tools as T  # noqa: E402

DEV = torch.device("cuda:0")
PW = 2.13
SHAPES = [(3, 63), (3, 2500), (2, 40000)]  # under one vector; one block and a ragged tail; several blocks
RTOL, ATOL = 2e-6, 1e-7


def _data(batch, per_sample, dtype, seed=0):
    g = torch.Generator().manual_seed(seed + per_sample)
    x = (torch.randn(batch, 1, per_sample, generator=g) * 2.0).to(dtype)
    t = (torch.rand(batch, 1, per_sample, generator=g) < 0.03).float()
    return x, t


def _reference(x, t, nv):
    """fp64 on the CPU, from the logits the kernel sees (a bf16 logit is its exact value)."""
    xs, ts = x[:nv].double(), t[:nv].double()
    if nv == 0:
        return 0.0, 0, 0
    loss = F.binary_cross_entropy_with_logits(xs, ts, pos_weight=torch.tensor([PW], dtype=torch.float64),
                                              reduction="sum").item() / x[0].numel()
    p, q = xs > 0, ts != 0
    return loss, int((p & q).sum()), int((p | q).sum())


def _check(totals, want, scale=1):
    got = totals.tolist()
    print(f"got {got} want {[w * scale for w in want]}")
    assert got[0] == pytest.approx(want[0] * scale, rel=RTOL, abs=ATOL)
    assert got[1] == want[1] * scale and got[2] == want[2] * scale


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("batch,per_sample", SHAPES)
def test_val_accumulate_matches_fp64_reference(dtype, batch, per_sample):
    x, t = _data(batch, per_sample, dtype)
    xd, td = x.to(DEV), t.to(DEV)
    for nv in (0, 1, batch, None):
        want = _reference(x, t, batch if nv is None else nv)
        n_valid = None if nv is None else torch.tensor([nv], device=DEV, dtype=torch.int32)
        totals = torch.zeros(3, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=PW)
        _check(totals, want)
        first = totals.clone()
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=PW)  # a second call adds to the totals
        _check(totals, want, scale=2)
        again = torch.zeros(3, device=DEV, dtype=torch.float64)
        T.val_accumulate(xd, td, again, n_valid=n_valid, pos_weight=PW)  # fixed order: bit-equal
        assert torch.equal(again, first)


def test_val_accumulate_misaligned_logits():
    """Logits and labels that are not 16-byte aligned take the per-element loads."""
    batch, per_sample = 3, 2500
    x, t = _data(batch, per_sample, torch.float32, seed=5)
    xd = torch.empty(x.numel() + 1, device=DEV)[1:].view_as(x).copy_(x)
    td = torch.empty(t.numel() + 1, device=DEV)[1:].view_as(t).copy_(t)
    assert xd.data_ptr() % 16 != 0
    totals = torch.zeros(3, device=DEV, dtype=torch.float64)
    T.val_accumulate(xd, td, totals, pos_weight=PW)
    _check(totals, _reference(x, t, batch))


def test_captured_val_accumulate_follows_n_valid():
    batch, per_sample = 3, 2500
    x, t = _data(batch, per_sample, torch.bfloat16, seed=9)
    xd, td = x.to(DEV), t.to(DEV)
    n_valid = torch.tensor([batch], device=DEV, dtype=torch.int32)
    totals = torch.zeros(3, device=DEV, dtype=torch.float64)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=PW)  # the scratch exists before the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        T.val_accumulate(xd, td, totals, n_valid=n_valid, pos_weight=PW)
    for nv in (batch, 1, 0, 2):
        totals.zero_()
        n_valid.fill_(nv)
        graph.replay()
        _check(totals, _reference(x, t, nv))
