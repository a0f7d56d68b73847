"""Float64 truth of the flat optimizer (csrc/jh_rbnet.hip: jh_rb_gradnorm_kernel + jh_rb_optim_kernel<Adam | RMSprop>, entered through
jh_rbnet_optim_step and jh_flat_adam_step) on ONE flat vector, and the size ladder that walks the two kernels' launch edges.

Truth: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam / torch.optim.RMSprop (plain and centered) on a single float64 CPU
tensor, with a torch-CPU float32 twin beside it the way fp64_truth.OptimTruth pairs them.  The starting state (params, m, v, step count) can
be given, so one step from anywhere in a run is checked without running up to it.  The criteria are fp64_truth.check_flat_step's.

Test infrastructure, not the product."""
import os

import torch

import fp64_truth as T

# ---------------------------------------------------------------------------------------------- launch constants (named here, once)
# csrc/jh_rbnet.hip: the launches at the end of the file (lines 1490-1513), jh_rbnet_optim_step / jh_flat_adam_step ("JH_LAUNCH(jh_rb_optim_kernel<..>, dim3(kOptGrid + f.extra_wgs), dim3(256), ..." and
# "JH_LAUNCH(jh_rb_gradnorm_kernel, dim3(256), dim3(256), ..."), and the loops of the two kernels (lines 479-492 and 581-592):
#   optimizer: `for (i = blockIdx.x * 256 + threadIdx.x; i < n4; i += main_wgs * 256)` over float4s
#   norm:      `for (; i + 3 * stride < n4; i += 4 * stride)` (four loads in flight), then `for (; i < n4; i += stride)`, stride = gridDim.x * 256
LANES = 256        # lanes of a workgroup, both kernels
VEC = 4            # floats per access (float4)
OPT_WGS = 512      # workgroups of the optimizer kernel (kOptGrid's default)
NORM_WGS = 256     # workgroups of the norm kernel
NORM_UNROLL = 4    # rounds the norm kernel's first loop takes at once


def opt_wgs(environ=None):
    """The optimizer's grid the way the library reads it: `getenv("JH_RB_OPTIM_GRID") ? atoi(...) : 512`."""
    env = (os.environ if environ is None else environ).get("JH_RB_OPTIM_GRID")
    if env is None:
        return OPT_WGS
    digits = env.strip()
    k = 1 if digits[:1] in "+-" else 0
    while k < len(digits) and digits[k].isdigit():
        k += 1
    try:
        return int(digits[:k])
    except ValueError:
        return 0  # atoi of no number


def edges():
    """The sizes, in float4s, at which another set of lanes runs another loop."""
    opt_pass = opt_wgs() * LANES            # one grid pass of the optimizer
    norm_stride = NORM_WGS * LANES          # one round of the norm kernel
    return dict(wave=64, workgroup=LANES, opt_pass=opt_pass, norm_first_unroll=(NORM_UNROLL - 1) * norm_stride, norm_all_unroll=NORM_UNROLL * norm_stride,
                norm_stride=norm_stride)


# RainbowNet kind "q", mlp head, S = 4, A = 2: n_params = H^2 + 8 H + 4 (w1 4H, b1 H, wl H^2, bl H, q 2H, its bias 2 -> 4).
LADDER_S, LADDER_A = 4, 2
# H -> (what it reaches, predicate on n4 = n_params / 4 and edges())
LADDER = {
    4: ("a fraction of one wave", lambda n4, e: 0 < n4 < e["wave"]),
    28: ("under one workgroup, its last wave ragged", lambda n4, e: e["workgroup"] - e["wave"] < n4 < e["workgroup"]),
    32: ("two workgroups", lambda n4, e: e["workgroup"] < n4 <= 2 * e["workgroup"]),
    720: ("just under one full grid pass of the optimizer: its last workgroup is ragged", lambda n4, e: e["opt_pass"] - e["workgroup"] < n4 < e["opt_pass"]),
    724: ("just over it: a second grid-stride round for some lanes", lambda n4, e: e["opt_pass"] < n4 < e["opt_pass"] + e["opt_pass"] // 8),
    880: ("just under the norm kernel's first unrolled round: no lane unrolls", lambda n4, e: 0.99 * e["norm_first_unroll"] < n4 <= e["norm_first_unroll"]),
    884: ("just over it: only some lanes unroll", lambda n4, e: e["norm_first_unroll"] < n4 < 1.01 * e["norm_first_unroll"]),
    1024: ("every lane unrolls once, some take a remainder round", lambda n4, e: e["norm_all_unroll"] < n4 < e["norm_all_unroll"] + e["norm_stride"]),
}


# ---------------------------------------------------------------------------------------------- the truth
OPTS = ("adam", "rmsprop", "rmsprop_centered")


def clip_coef64(g, max_norm):
    """clip_grad_norm_'s coefficient in float64: min(1, max_norm / (|g| + 1e-6)).  -> (coef, norm)"""
    norm = float(torch.as_tensor(g).detach().double().cpu().norm())
    return min(1.0, float(max_norm) / (norm + 1e-6)), norm


class _Run:
    """One dtype's run: a single flat parameter, its torch.optim optimizer, and a state that can be set."""

    def __init__(self, opt, n, dtype, lr, beta1, beta2, eps):
        self.opt_name, self.dtype = opt, dtype
        self.p = torch.nn.Parameter(torch.zeros(n, dtype=dtype))
        if opt == "adam":
            self.opt = torch.optim.Adam([self.p], lr=lr, betas=(beta1, beta2), eps=eps)
            self.keys = ("exp_avg", "exp_avg_sq")
        else:
            self.opt = torch.optim.RMSprop([self.p], lr=lr, alpha=beta1, eps=eps, centered=opt == "rmsprop_centered")
            self.keys = ("grad_avg" if opt == "rmsprop_centered" else None, "square_avg")
        # torch creates the state in its first step; a step on a zero gradient from a zero state creates it and moves nothing
        self.p.grad = torch.zeros_like(self.p)
        self.opt.step()
        assert not self.p.detach().any()

    def set_state(self, params, m, v, step):
        st = self.opt.state[self.p]
        with torch.no_grad():
            self.p.copy_(params.to(self.dtype))
            if self.keys[0] is not None:
                st[self.keys[0]].copy_(m.to(self.dtype))
            st[self.keys[1]].copy_(v.to(self.dtype))
            if torch.is_tensor(st["step"]):
                st["step"].fill_(float(step))
            else:
                st["step"] = int(step)

    def step(self, g, max_norm):
        """-> gradient as the optimizer saw it (clipped in place, like p.grad in the reference)"""
        self.p.grad = g.detach().to(self.dtype).clone()
        if max_norm:
            torch.nn.utils.clip_grad_norm_([self.p], max_norm)
        self.opt.step()
        return self.p.grad.detach().clone()

    def state(self):
        st = self.opt.state[self.p]
        return dict(params=self.p.detach().clone(), m=st[self.keys[0]].clone() if self.keys[0] is not None else None, v=st[self.keys[1]].clone(),
                    step=int(st["step"]))


class FlatTruth:
    """clip_grad_norm_ + one optimizer on a flat vector, in float64 (`r64`) and torch-CPU float32 (`r32`).  beta1 is RMSprop's alpha.  The
    starting state (flat tensors of any float dtype, None = zeros) is rounded to float32 first: it is what a float32 implementation starts from."""

    def __init__(self, opt, n, lr, beta1=0.9, beta2=0.999, eps=1e-8, params=None, m=None, v=None, step=0):
        assert opt in OPTS, opt
        self.opt, self.lr, self.n = opt, lr, n
        self.r64, self.r32 = (_Run(opt, n, dt, lr, beta1, beta2, eps) for dt in (torch.float64, torch.float32))
        z = torch.zeros(n)
        f32 = lambda t: z if t is None else torch.as_tensor(t).detach().cpu().float().reshape(n)
        for r in (self.r64, self.r32):
            r.set_state(f32(params), f32(m), f32(v), step)

    def set_lr(self, lr):
        self.lr = lr
        for r in (self.r64, self.r32):
            r.opt.param_groups[0]["lr"] = lr

    def step(self, g, max_norm=None):
        """Both runs take one step on the gradient g (each in its own dtype).  -> (before, after, g_seen): the float64 run's state() before
        and after, and the gradient as its optimizer saw it."""
        before = self.r64.state()
        seen = self.r64.step(torch.as_tensor(g).detach().cpu().reshape(self.n), max_norm)
        self.r32.step(torch.as_tensor(g).detach().cpu().reshape(self.n), max_norm)
        return before, self.r64.state(), seen

    def check(self, ours, before, after, tag, allowed=None):
        """ours: dict params / m / v of flat tensors after OUR step of the gradient the float64 run just took.  -> worst weight ratio."""
        moments = [(key, ours[name], after[name]) for key, name in zip(self.r64.keys, ("m", "v")) if key is not None]
        return T.check_flat_step(ours["params"], after["params"], before["params"], self.lr, f"{tag} weights", "vs float64 step of OUR gradient",
                                 moments=moments, moment_tag=f"{tag} {{key}}", allowed=allowed)
