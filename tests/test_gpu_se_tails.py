"""Squeeze-excite with the MLPs in the reductions' last blocks (lss_se_fwd / lss_se_bwd, two launches each)
against the earlier launch sequence (lss_se_tails(0)): every buffer of the C ABI, bit for bit. The tails are
forced (setting 2) so that every shape takes them, also those the default setting routes to the sequence."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

from lss_carla_amd import _lib  # noqa: E402
from lss_carla_amd import efficientnet as E  # noqa: E402

DEV = torch.device("cuda:0")
BANK_IMAGES = 4096  # LSS_SE_TAIL_MAX_IMAGES of include/lss_convs.h: one counter word per image

# (N, C, HW, sq) -- what each shape guards
SHAPES = [
    (1, 4, 4, 1),              # one block is the whole image
    (3, 6, 4, 1),              # C no multiple of the planes per block: a block must not straddle images
    (2, 72, 12, 3),            # HW % 8 == 4; a second 64-channel chunk with 8 live channels; odd sq
    (2, 320, 8, 5),            # two 256-channel expand chunks and five 64-channel backward chunks
    (5, 1152, 44, 48),         # the widest trunk block at its real plane size
    (1, 2048, 4, 64),          # the ABI's limits
    (48, 8, 4, 2),             # the workload's image count
    (BANK_IMAGES + 1, 4, 4, 1),  # past the counter bank: the fallback sequence
    # N * ceil(C / 16) past the 512 resident blocks: a block takes 32 or more channels and a wave several
    # planes, their loads batched (four at a time in the mean, two in the dot)
    (48, 240, 8, 10),          # 32 channels a block: every wave one full batch of two
    (64, 1152, 4, 48),         # 144 channels a block: mean batches of 4, 4, 1 planes, dot 2, 2, 2, 2, 1
    (40, 600, 12, 25),         # 64 channels a block, 24 in the last: waves 0-7 take two planes, 8-15 one
]

FWD = ("m", "r", "h", "sig", "y")
BWD = ("t", "de", "dr", "dm", "dx")
WGRAD = ("dw1", "db1", "dw2", "db2")


def _inputs(N, C, HW, sq, seed):
    g = torch.Generator().manual_seed(seed)
    d = {"x": (torch.randn(N, C, HW, generator=g) * 2).bfloat16(), "dy": torch.randn(N, C, HW, generator=g).bfloat16(),
         "w1": torch.randn(sq, C, generator=g) / C ** 0.5, "b1": torch.randn(sq, generator=g),
         "w2": torch.randn(C, sq, generator=g) / sq ** 0.5, "b2": torch.randn(C, generator=g)}
    return {k: v.to(DEV) for k, v in d.items()}


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


OFF, DEFAULT, FORCED = 0, 1, 2  # lss_se_tails settings


def _run(inp, tails):
    """Forward, backward and weight gradients through the C ABI under one lss_se_tails setting; every
    output buffer NaN-filled first. The previous setting is put back."""
    lib = _lib.load()
    N, C, HW = inp["x"].shape
    sq = inp["w1"].shape[0]
    o = {"m": _nan(N, C), "r": _nan(N, sq), "h": _nan(N, sq), "sig": _nan(N, C),
         "y": _nan(N, C, HW, dtype=torch.bfloat16), "t": _nan(N, C), "dh_part": _nan(N, (C + 63) // 64, sq),
         "de": _nan(N, C), "dr": _nan(N, sq), "dm": _nan(N, C), "dx": _nan(N, C, HW, dtype=torch.bfloat16),
         "dw1": _nan(sq, C), "db1": _nan(sq), "dw2": _nan(C, sq), "db2": _nan(C)}
    p, st = _lib.ptr, _lib.stream_handle(DEV)
    prev = lib.lss_se_tails(int(tails))
    try:
        _lib.check(lib.lss_se_fwd(p(inp["x"]), N, C, HW, p(inp["w1"]), p(inp["b1"]), p(inp["w2"]), p(inp["b2"]), sq,
                                  p(o["m"]), p(o["r"]), p(o["h"]), p(o["sig"]), p(o["y"]), st), "lss_se_fwd")
        _lib.check(lib.lss_se_bwd(p(inp["dy"]), p(inp["x"]), N, C, HW, p(inp["w1"]), p(inp["w2"]), sq, p(o["r"]),
                                  p(o["sig"]), p(o["t"]), p(o["dh_part"]), p(o["de"]), p(o["dr"]), p(o["dm"]),
                                  p(o["dx"]), st), "lss_se_bwd")
        _lib.check(lib.lss_se_wgrad(p(o["de"]), p(o["h"]), p(o["dr"]), p(o["m"]), N, C, sq, p(o["dw1"]), p(o["db1"]),
                                    p(o["dw2"]), p(o["db2"]), st), "lss_se_wgrad")
    finally:
        lib.lss_se_tails(prev)
    torch.cuda.synchronize()
    return o


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _assert_same(on, off, what=""):
    for k in FWD + BWD + WGRAD:
        assert not torch.isnan(off[k]).any(), (what, k, "fallback left NaN")
        assert torch.equal(_bits(on[k]), _bits(off[k])), (what, k, int((_bits(on[k]) != _bits(off[k])).sum()))


@pytest.mark.parametrize("N,C,HW,sq", SHAPES)
def test_tails_equal_the_launch_sequence_bit_for_bit(N, C, HW, sq):
    inp = _inputs(N, C, HW, sq, seed=C + HW)
    on, off = _run(inp, FORCED), _run(inp, OFF)
    _assert_same(on, off)
    _assert_same(_run(inp, DEFAULT), off, what="default setting")
    # The switch's documented behaviour: the tails leave dh_part untouched, the fallback sequence stores
    # the chunk partials in it -- also with the tails on, once N exceeds the counter bank.
    assert not torch.isnan(off["dh_part"]).any()
    if N > BANK_IMAGES:
        assert not torch.isnan(on["dh_part"]).any()
    else:
        assert torch.isnan(on["dh_part"]).all()


@pytest.mark.parametrize("N,C,HW,sq", [(3, 6, 4, 1), (2, 320, 8, 5)])
def test_counters_are_left_at_zero(N, C, HW, sq):
    """Three calls back to back, nothing reset between them: a counter left non-zero would hand an image's
    MLP to a block that is not the last (NaN or stale values), or to none."""
    inps = [_inputs(N, C, HW, sq, seed=100 + i) for i in range(3)]
    ons = [_run(inp, FORCED) for inp in inps]
    for i, inp in enumerate(inps):
        _assert_same(ons[i], _run(inp, OFF), what=f"call {i}")


def test_graph_replay_equals_eager():
    """One captured forward + backward of squeeze_excite replayed with fresh inputs: the counters end every
    replay at zero and the bank chosen at capture is reused, so each replay must equal the eager call --
    taken with the tails off, so that the reference shares nothing with what it checks."""
    N, C, H, W, sq = 6, 240, 16, 44, 10
    torch.manual_seed(3)
    red, exp = torch.nn.Conv2d(C, sq, 1).to(DEV), torch.nn.Conv2d(sq, C, 1).to(DEV)
    params = [red.weight, red.bias, exp.weight, exp.bias]
    g = torch.Generator().manual_seed(4)

    def fresh():
        return ((torch.randn(N, C, H, W, generator=g) * 2).bfloat16().to(DEV),
                torch.randn(N, C, H, W, generator=g).bfloat16().to(DEV))

    def step(x, dy):
        y = E.squeeze_excite(x, red, exp)
        return (y,) + torch.autograd.grad(y, [x] + params, dy)

    prev = _lib.load().lss_se_tails(FORCED)  # C * sq = 2400: the default would take the forward's launch sequence
    try:
        _graph_replay(step, fresh)
    finally:
        _lib.load().lss_se_tails(prev)


def _graph_replay(step, fresh):
    x0, dy0 = fresh()
    xs, dys = x0.clone().requires_grad_(True), dy0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(xs, dys)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step(xs, dys)
    for _ in range(3):
        x, dy = fresh()
        with torch.no_grad():
            xs.copy_(x)
            dys.copy_(dy)
        graph.replay()
        torch.cuda.synchronize()
        forced = _lib.load().lss_se_tails(OFF)
        try:
            want = step(x.requires_grad_(True), dy)
        finally:
            _lib.load().lss_se_tails(forced)
        for a, b in zip(outs, want):
            assert not torch.isnan(b.float()).any()
            assert torch.equal(_bits(a), _bits(b.detach()))
