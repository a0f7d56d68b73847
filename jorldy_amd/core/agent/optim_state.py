"""The one mapping between native optimizer moments and a torch.optim state_dict (the "optimizer" entries of the reference's ckpt): which
entry names Adam and RMSprop use, which parameters have an entry, how the step count and param_groups[0] come back.  Everything works on
lists of tensors in parameter order; where the tensors come from and go to (buckets, views, device blocks) is the caller's business."""
import torch

from ..optimizer import Optimizer


def _entries(opt):
    """(entry of the first moment or None, entry of the second) in the order torch's own step() creates them after "step"."""
    if isinstance(opt, torch.optim.RMSprop):
        return ("grad_avg" if opt.defaults["centered"] else None), "square_avg"
    return "exp_avg", "exp_avg_sq"


def shadow(optim_config, tensors, lr):
    """-> (opt, params): the configured torch optimizer over Parameters made from `tensors`, every group's lr set to `lr`."""
    params = [torch.nn.Parameter(t) for t in tensors]
    opt = Optimizer(**optim_config, params=params)
    for grp in opt.param_groups:
        grp["lr"] = lr
    return opt, params


def fill(opt, params, steps, m, v):
    """opt.state[params[i]] <- {step, m[i], v[i]}; v[i] None: no entry, as torch's own optimizer has it for a parameter that never took a step."""
    km, kv = _entries(opt)
    for p, mi, vi in zip(params, m, v):
        if vi is None:
            opt.state.pop(p, None)
            continue
        pairs = [(km, mi), (kv, vi)] if km == "exp_avg" else [(kv, vi), (km, mi)]
        opt.state[p] = {"step": torch.tensor(float(steps)), **{k: t for k, t in pairs if k}}


def read(opt, params):
    """-> (steps, m, v): the lists aligned with `params`, None where the optimizer holds no state (every m[i] for a non-centered RMSprop);
    steps from the first parameter that has state, 0 if none has."""
    km, kv = _entries(opt)
    held = [opt.state.get(p) or None for p in params]
    steps = next((int(float(s["step"])) for s in held if s), 0)
    return steps, [s[km] if s and km else None for s in held], [s[kv] if s else None for s in held]


def dense(moments, like):
    """The rule for writing back into native memory: a parameter without an entry gets zero moments."""
    return [torch.zeros_like(p) if t is None else t for t, p in zip(moments, like)]


def hyper(group):
    """A param group (or an optimizer's defaults) -> (lr, beta1, beta2, eps, centered) as the native set_hyper calls take them; RMSprop's
    alpha stands in beta1's place."""
    b1, b2 = group["betas"] if "betas" in group else (group["alpha"], 0.0)
    return float(group["lr"]), b1, b2, group["eps"], bool(group.get("centered", False))
