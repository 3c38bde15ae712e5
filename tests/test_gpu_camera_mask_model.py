"""``LiftSplatShoot.camera_alive`` and ``Predictor(camera_mask=True)`` at final_dim (64, 192), bsz 2: a forward with
dead cameras equals, bit for bit, the forward on a rig whose dead cameras are moved 1e6 m away (every one of their
frustum points out of the grid: same shapes, same trunk, same kernels but the plan's) -- eager, as one captured
graph replayed under changing masks, and in train mode through the backward. cudnn.deterministic is on as in
tests/test_gpu_predict.py: the comparison is of two forwards."""
import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():
    pytest.skip("needs an MI355X", allow_module_level=True)

import lss_carla_amd as L  # noqa: E402
from lss_carla_amd import synthetic as syn  # noqa: E402

DEV = torch.device("cuda:0")
BF16 = torch.bfloat16
GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
B, N = 2, 6
RIG = ("rots", "trans", "intrins", "post_rots", "post_trans")
ALIVE = torch.tensor([[1, 0, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0]], dtype=torch.uint8)  # per sample


@pytest.fixture(scope="module", autouse=True)
def _deterministic():
    old = torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = False, True
    yield
    torch.backends.cudnn.benchmark, torch.backends.cudnn.deterministic = old


def _model(seed):
    torch.manual_seed(seed)
    m = L.compile_model(GC, DAC, outC=1).to(DEV)
    m.bevencode.to(memory_format=torch.channels_last)
    m.camencode.up1.to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # running statistics a trained network would have (fresh ones are 0 / 1)
        for bn in (x for x in m.modules() if isinstance(x, nn.BatchNorm2d)):
            bn.running_mean.copy_(torch.empty(bn.num_features).normal_(0, 0.1, generator=g))
            bn.running_var.copy_(torch.empty(bn.num_features).uniform_(0.5, 1.5, generator=g))
    return m.train()


def _inputs(seed, alive=None):
    """Host inputs; with `alive`, the dead cameras' trans moved 1e6 m away."""
    rig = syn.make_rig(B, N, DAC["final_dim"], seed=seed)
    if alive is not None:
        rig["trans"] = rig["trans"].clone()
        rig["trans"][alive == 0] += 1.0e6
    return (syn.make_images(B, N, DAC["final_dim"], seed=seed), *(rig[k] for k in RIG))


def _eager_eval(model, inputs, alive=None):
    was, saved = model.training, model.camera_alive
    model.eval()
    model.camera_alive = None if alive is None else alive.to(DEV).contiguous()
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=BF16):
            return model(*(t.to(DEV) for t in inputs))
    finally:
        model.camera_alive = saved
        model.train(was)


def test_default_is_none_and_forward_keeps_its_signature():
    import inspect
    m = _model(0)
    assert m.camera_alive is None
    assert list(inspect.signature(m.forward).parameters) == ["x", "rots", "trans", "intrins", "post_rots", "post_trans"]


def test_eval_forward_with_a_mask_equals_the_far_away_rig_eager_and_replayed():
    model = _model(1)
    plain = _eager_eval(model, _inputs(5))
    far = _eager_eval(model, _inputs(5, ALIVE))
    got = _eager_eval(model, _inputs(5), ALIVE)
    assert torch.isfinite(far.float()).all() and not torch.equal(far, plain)
    assert torch.equal(got, far), (got.float() - far.float()).abs().max().item()
    assert torch.equal(_eager_eval(model, _inputs(5), torch.ones(B, N, dtype=torch.uint8)), plain)
    assert model.camera_alive is None

    p = L.Predictor(model, B, DEV, amp_dtype=BF16, graph=True, camera_mask=True)
    assert p.alive.shape == (B, N) and p.alive.dtype == torch.uint8 and bool(p.alive.all())
    first = p(*_inputs(5)).clone()  # all ones: captures the masked graph
    graph = p.graph
    assert graph is not None and torch.equal(first, plain)
    assert torch.equal(p(*_inputs(5), alive=ALIVE), far)            # per call, (b, N)
    one = torch.tensor([1, 1, 0, 1, 1, 1], dtype=torch.bool)        # (N,): every sample
    p.set_alive(one)
    want_one = _eager_eval(model, _inputs(5, one.expand(B, N)))
    assert torch.equal(p(*_inputs(5)), want_one) and not torch.equal(want_one, far)
    assert torch.equal(p(*_inputs(5), alive=ALIVE.to(DEV)), far)    # a device mask
    p.set_alive(np.ones(N, dtype=np.uint8))
    assert torch.equal(p(*_inputs(5)), first)                       # back to all ones: the first output again
    assert p.graph is graph, "one captured graph serves every pattern"
    assert model.camera_alive is None and model.training
    with pytest.raises(ValueError):
        p.set_alive([1, 0, 1])


def test_a_predictor_without_camera_mask_refuses_alive():
    model = _model(2)
    p = L.Predictor(model, B, DEV, amp_dtype=BF16, graph=False)
    assert p.alive is None
    with pytest.raises(RuntimeError, match="camera_mask"):
        p(*_inputs(1), alive=ALIVE)
    with pytest.raises(RuntimeError, match="camera_mask"):
        p.set_alive(ALIVE)
    out = p(*_inputs(1))  # and it still runs, unmasked
    assert torch.equal(out, _eager_eval(model, _inputs(1)))


def test_train_mode_forward_backward_with_a_mask_matches_the_far_away_rig():
    model = _model(3)
    labels = syn.make_labels(B, 200, 200, seed=1).to(DEV)

    def run(inputs, alive):
        model.zero_grad(set_to_none=True)
        model.camera_alive = None if alive is None else alive.to(DEV).contiguous()
        torch.manual_seed(11)  # the dropouts' draws
        torch.cuda.manual_seed(11)
        try:
            with torch.autocast("cuda", dtype=BF16):
                preds = model(*(t.to(DEV) for t in inputs))
            loss = nn.functional.binary_cross_entropy_with_logits(preds.float(), labels)
            loss.backward()
        finally:
            model.camera_alive = None
        torch.cuda.synchronize()
        return preds.detach().clone(), {k: v.grad.detach().clone() for k, v in model.named_parameters()
                                        if v.grad is not None}

    p_far, g_far = run(_inputs(6, ALIVE), None)
    p_got, g_got = run(_inputs(6), ALIVE)
    p_all, _ = run(_inputs(6), None)
    assert not torch.equal(p_far, p_all)
    assert torch.equal(p_got, p_far)
    assert len(g_far) > 100 and set(g_got) == set(g_far)
    for k, v in g_far.items():
        assert torch.equal(g_got[k], v), k
    assert any(v.any() for v in g_far.values())
