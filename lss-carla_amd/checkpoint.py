"""Checkpoints in the reference's format (train_simbev.py:422-453, read back at 203-213) from flat masters.

The reference saves ``model.state_dict()`` and the ``state_dict()`` of
``torch.optim.Adam(model.parameters(), ...)``: optimizer state keyed by each parameter's position in
``model.parameters()``. Here the optimizer sees one flat fp32 master per parameter group
(flat_params.FlatParams / FlatParamGroups) whose Adam state is flat too, so ``save_checkpoint`` writes the
per-parameter views of that state under the reference's indices -- a file either trainer can resume from --
and ``load_checkpoint`` scatters such a file back into the flat tensors in place: captured graphs hold
their addresses.

Parameters that never receive a gradient carry no optimizer state, as in torch: the constants ``dx``,
``bx``, ``nx``, ``frustum`` (nn.Parameters without requires_grad, src/models.py:143-152) and whatever
``parallel.freeze_unused`` froze (EfficientNet's unused head) take an index and nothing else.

When the flat parameters keep an EMA of the weights (``enable_ema``), the file gains one key, ``ema_state_dict``: a
full state dict the reference's ``model.load_state_dict`` can load as it is. ``load_checkpoint`` copies it into the
EMA tensors in place; a file without it starts the EMA from the loaded weights and says so.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch


def _groups(flat) -> list:
    return list(flat.groups) if hasattr(flat, "groups") else [flat]


def _masters(flat) -> List[torch.Tensor]:
    return [g.master for g in _groups(flat)]


def _indices(model: torch.nn.Module) -> Dict[str, int]:
    return {name: i for i, (name, _) in enumerate(model.named_parameters())}


def _check(flat, opt) -> None:
    ps = [p for g in opt.param_groups for p in g["params"]]
    ms = _masters(flat)
    if len(opt.param_groups) != 1 or len(ps) != len(ms) or any(a is not b for a, b in zip(ps, ms)):
        raise ValueError("checkpoint: the optimizer must hold exactly the flat masters, in one parameter group")


def optimizer_state_dict(model: torch.nn.Module, flat, opt: torch.optim.Optimizer) -> dict:
    """What ``torch.optim.Adam(model.parameters(), ...).state_dict()`` would hold after the same steps."""
    _check(flat, opt)
    index = _indices(model)
    state = {}
    for grp in _groups(flat):
        st = opt.state.get(grp.master, {})
        if not st:
            continue  # no step taken yet: torch has no entry either
        step = torch.as_tensor(st["step"]).detach().to("cpu", torch.float32).reshape(())
        avg, sq = grp.views_of(st["exp_avg"].detach()), grp.views_of(st["exp_avg_sq"].detach())
        for name in avg:
            state[index[name]] = {"step": step.clone(), "exp_avg": avg[name].contiguous().clone(),
                                  "exp_avg_sq": sq[name].contiguous().clone()}
    g = opt.param_groups[0]
    # the keys, and the defaults of those this trainer does not set, of a plain torch Adam
    proto = torch.optim.Adam([torch.zeros(1)], lr=float(g["lr"]), betas=tuple(float(b) for b in g["betas"]),
                             eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
    group = dict(proto.state_dict()["param_groups"][0])
    group["params"] = list(range(len(index)))
    return {"state": dict(sorted(state.items())), "param_groups": [group]}


def save_checkpoint(path, model: torch.nn.Module, flat, opt: torch.optim.Optimizer, counter: int, epoch: int,
                    val_iou: Optional[float] = None) -> dict:
    """Write the reference's checkpoint dict; returns it. (Reads the device: call it at the loop's own
    checkpoint cadence.)"""
    ckpt = {
        "model_state_dict": model.state_dict(),  # the module's own: its parameters alias the masters
        "optimizer_state_dict": optimizer_state_dict(model, flat, opt),
        "counter": int(counter),
        "epoch": int(epoch),
    }
    if val_iou is not None:
        ckpt["val_iou"] = float(val_iou)
    if _has_ema(flat):
        ckpt["ema_state_dict"] = ema_state_dict(model, flat)
    torch.save(ckpt, path)
    return ckpt


def _has_ema(flat) -> bool:
    return all(getattr(g, "ema", None) is not None for g in _groups(flat))


def ema_state_dict(model: torch.nn.Module, flat) -> dict:
    """A full state dict with the EMA values for the trainable parameters and the live values for everything
    else (frozen parameters, constants, batch-norm statistics): ``model.load_state_dict`` loads it as it is."""
    sd = dict(model.state_dict())
    for grp in _groups(flat):
        for name, view in grp.views_of(grp.ema).items():
            if name not in sd:
                raise KeyError(f"checkpoint: {name} is not a key of the model's state dict")
            sd[name] = view.detach().clone()
    return sd


def load_ema(sd: Optional[dict], flat) -> None:
    """Copy an ``ema_state_dict`` into the EMA tensors in place; None (a file without one): the EMA starts from
    the current weights."""
    with torch.no_grad():
        for grp in _groups(flat):
            if sd is None:
                grp.ema.copy_(grp.master.detach())
                continue
            for name, view in grp.views_of(grp.ema).items():
                view.copy_(sd[name])


def init_state(opt: torch.optim.Optimizer, master: torch.Tensor) -> dict:
    """The optimizer's state of one flat master, created (zeros) if it has none yet: a caller that captures
    the update needs the state tensors at their final addresses before the capture."""
    st = opt.state[master]
    if len(st) == 0:  # as torch.optim.Adam creates it (capturable / fused: the step on the device)
        g = opt.param_groups[0]
        on_dev = bool(g.get("capturable") or g.get("fused"))
        st["step"] = torch.zeros((), dtype=torch.float32, device=master.device if on_dev else "cpu")
        st["exp_avg"] = torch.zeros_like(master, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(master, memory_format=torch.preserve_format)
    return st


def load_optimizer_state(sd: dict, model: torch.nn.Module, flat, opt: torch.optim.Optimizer) -> None:
    """Scatter a per-parameter Adam state dict (this module's or the reference's) into the flat state
    tensors in place; parameters without an entry get zero moments."""
    _check(flat, opt)
    index = _indices(model)
    entries = {int(k): v for k, v in sd.get("state", {}).items()}
    with torch.no_grad():
        for grp in _groups(flat):
            st = init_state(opt, grp.master)
            avg, sq = grp.views_of(st["exp_avg"]), grp.views_of(st["exp_avg_sq"])
            steps = []
            for name in avg:
                e = entries.get(index[name])
                if e is None:
                    avg[name].zero_()
                    sq[name].zero_()
                    continue
                avg[name].copy_(e["exp_avg"])
                sq[name].copy_(e["exp_avg_sq"])
                steps.append(float(torch.as_tensor(e["step"]).item()))
            if steps and min(steps) != max(steps):
                raise ValueError(f"checkpoint: parameters of one flat group at different steps ({min(steps)}, {max(steps)})")
            if torch.is_tensor(st["step"]):
                st["step"].fill_(steps[0] if steps else 0.0)
            else:
                st["step"] = steps[0] if steps else 0.0


def load_checkpoint(path, model: torch.nn.Module, flat, opt: torch.optim.Optimizer) -> Tuple[int, int]:
    """Load a checkpoint written here or by the reference, or a bare model state dict
    (train_simbev.py:206-212), in place; returns (counter, epoch) -- (0, 0) for a bare state dict."""
    dev = _masters(flat)[0].device
    ckpt = torch.load(path, map_location=dev)
    if isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        model.load_state_dict(ckpt["model_state_dict"])  # copies into the parameters: the masters' memory
        load_optimizer_state(ckpt["optimizer_state_dict"], model, flat, opt)
        if _has_ema(flat):
            if "ema_state_dict" not in ckpt:
                print(f"{path} has no ema_state_dict: the EMA starts from the loaded weights")
            load_ema(ckpt.get("ema_state_dict"), flat)
        return int(ckpt.get("counter", 0)), int(ckpt.get("epoch", 0))
    model.load_state_dict(ckpt)
    if _has_ema(flat):
        print(f"{path} is a bare state dict: the EMA starts from the loaded weights")
        load_ema(None, flat)
    return 0, 0
