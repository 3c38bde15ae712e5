"""checkpoint.save_checkpoint / load_checkpoint on the CPU: the file written from flat masters is the
reference's (train_simbev.py:422-453) -- its optimizer state loads into, and matches entry by entry, a
plain ``torch.optim.Adam(model.parameters())`` fed the same gradients -- and loading it back into a fresh
flat setup continues the same trajectory. No forward pass is needed: the gradients are drawn."""
import copy

import pytest
import torch

import lss_carla_amd as L
from lss_carla_amd import checkpoint, parallel
from lss_carla_amd.flat_params import FlatParamGroups, FlatParams, lss_backward_groups

GC = {"xbound": [-50.0, 50.0, 0.5], "ybound": [-50.0, 50.0, 0.5], "zbound": [-10.0, 10.0, 20.0],
      "dbound": [4.0, 45.0, 1.0]}
DAC = {"resize_lim": (1.6, 1.8), "final_dim": (64, 192), "rot_lim": (-5.4, 5.4), "H": 56, "W": 120,
       "rand_flip": True, "bot_pct_lim": (0.0, 0.22), "Ncams": 6}
LR, WD = 1e-3, 1e-7
RTOL, ATOL = 1e-6, 1e-9  # fp32 Adam arithmetic, elementwise the same on both sides


@pytest.fixture(scope="module")
def initial():
    torch.manual_seed(0)
    model = L.compile_model(GC, DAC, outC=1)
    parallel.freeze_unused(model)
    return model


def _flat_setup(initial, grouped):
    model = copy.deepcopy(initial)
    flat = FlatParamGroups(model, lss_backward_groups()) if grouped else FlatParams(model)
    masters = flat.masters if grouped else [flat.master]
    return model, flat, masters, torch.optim.Adam(masters, lr=LR, weight_decay=WD)


def _step(flat, masters, opt, plain_model, plain_opt, gen):
    """One Adam step on both sides from the same drawn gradients."""
    groups = flat.groups if hasattr(flat, "groups") else [flat]
    plain = dict(plain_model.named_parameters())
    for grp, m in zip(groups, masters):
        m.grad = torch.randn(m.shape, generator=gen)
        for name, view in grp.views_of(m.grad).items():
            plain[name].grad = view.clone()
    opt.step()
    plain_opt.step()


@pytest.mark.parametrize("grouped", [True, False], ids=["FlatParamGroups", "FlatParams"])
def test_checkpoint_is_the_reference_format_and_round_trips(initial, grouped, tmp_path):
    model, flat, masters, opt = _flat_setup(initial, grouped)
    plain_model = copy.deepcopy(initial)
    plain_opt = torch.optim.Adam(plain_model.parameters(), lr=LR, weight_decay=WD)
    gen = torch.Generator().manual_seed(11)
    for _ in range(2):
        _step(flat, masters, opt, plain_model, plain_opt, gen)
    path = tmp_path / "model_000002.pt"
    checkpoint.save_checkpoint(path, model, flat, opt, counter=2, epoch=1, val_iou=0.25)
    ckpt = torch.load(path, map_location="cpu")
    assert set(ckpt) == {"model_state_dict", "optimizer_state_dict", "counter", "epoch", "val_iou"}
    assert (ckpt["counter"], ckpt["epoch"], ckpt["val_iou"]) == (2, 1, 0.25)
    assert list(ckpt["model_state_dict"]) == list(plain_model.state_dict())
    for k, v in plain_model.state_dict().items():
        torch.testing.assert_close(ckpt["model_state_dict"][k], v, rtol=RTOL, atol=ATOL)

    # the optimizer state: what the plain Adam holds, entry by entry
    got, want = ckpt["optimizer_state_dict"], plain_opt.state_dict()
    assert set(got) == set(want) == {"state", "param_groups"}
    assert len(got["param_groups"]) == 1 and set(got["param_groups"][0]) == set(want["param_groups"][0])
    for k, v in want["param_groups"][0].items():
        assert got["param_groups"][0][k] == v, k
    assert set(got["state"]) == set(want["state"])
    for i, w in want["state"].items():
        e = got["state"][i]
        assert set(e) == set(w) == {"step", "exp_avg", "exp_avg_sq"}
        assert e["step"].device.type == "cpu" and e["step"].dtype == torch.float32 and e["step"].dim() == 0
        assert float(e["step"]) == float(w["step"]) == 2.0
        assert e["exp_avg"].shape == w["exp_avg"].shape and e["exp_avg"].is_contiguous()
        torch.testing.assert_close(e["exp_avg"], w["exp_avg"], rtol=RTOL, atol=ATOL)
        torch.testing.assert_close(e["exp_avg_sq"], w["exp_avg_sq"], rtol=RTOL, atol=ATOL)
    # the constants and the frozen head take indices and carry no state
    names = [n for n, _ in model.named_parameters()]
    for n in ("dx", "bx", "nx", "frustum"):
        assert n in names and names.index(n) not in got["state"]
    frozen = [i for i, (n, p) in enumerate(model.named_parameters()) if not p.requires_grad]
    assert len(frozen) > 4 and not set(frozen) & set(got["state"])
    assert set(got["state"]) == {i for i, (n, p) in enumerate(model.named_parameters()) if p.requires_grad}
    # and it loads into a plain Adam over a plain model, as the reference's resume does
    other = copy.deepcopy(initial)
    other_opt = torch.optim.Adam(other.parameters(), lr=LR, weight_decay=WD)
    other.load_state_dict(ckpt["model_state_dict"])
    other_opt.load_state_dict(got)
    assert set(other_opt.state_dict()["state"]) == set(want["state"])

    # round trip into a fresh flat setup, in place, then one more step on both sides
    model2, flat2, masters2, opt2 = _flat_setup(initial, grouped)
    opt2.zero_grad()
    ptrs = [m.data_ptr() for m in masters2]
    assert checkpoint.load_checkpoint(path, model2, flat2, opt2) == (2, 1)
    assert [m.data_ptr() for m in masters2] == ptrs
    for m, m2 in zip(masters, masters2):
        assert torch.equal(m.detach(), m2.detach())
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[m][k], opt2.state[m2][k])
        assert float(opt2.state[m2]["step"]) == 2.0
    state_ptrs = [opt2.state[m]["exp_avg"].data_ptr() for m in masters2]
    assert checkpoint.load_checkpoint(path, model2, flat2, opt2) == (2, 1)  # existing state: in place
    assert [opt2.state[m]["exp_avg"].data_ptr() for m in masters2] == state_ptrs
    _step(flat2, masters2, opt2, plain_model, plain_opt, gen)
    want_sd = plain_model.state_dict()
    for k, v in model2.state_dict().items():
        torch.testing.assert_close(v, want_sd[k], rtol=RTOL, atol=ATOL)


def test_bare_state_dict_loads(initial, tmp_path):
    model, flat, masters, opt = _flat_setup(initial, True)
    src = copy.deepcopy(initial)
    with torch.no_grad():
        for p in src.parameters():
            if p.requires_grad:
                p.add_(0.5)
    path = tmp_path / "bare.pt"
    torch.save(src.state_dict(), path)
    ptrs = [m.data_ptr() for m in masters]
    assert checkpoint.load_checkpoint(path, model, flat, opt) == (0, 0)
    assert [m.data_ptr() for m in masters] == ptrs
    for (k, v), w in zip(model.state_dict().items(), src.state_dict().values()):
        assert torch.equal(v, w), k
    # the masters hold what was loaded (the parameters alias them)
    for name, view in flat.views().items():
        assert torch.equal(view, src.state_dict()[name])
