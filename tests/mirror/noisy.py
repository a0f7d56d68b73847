"""Forward-capable restatement of the reference's NoisyNet Q-network (core/network/noisy.py:8-50 on utils.py:55-86) -- TEST INFRASTRUCTURE like
mirror/networks.py: the container the product ships (jorldy_amd.core.network.Noisy: names, shapes, initialisation) plus `forward`, evaluated
on the CPU in float64 / float32 by the parity tests.  `noise` injects the Gaussian draws: {"l1": (e_in [F], e_out [H]), "l2": (e_in [H],
e_out [A])} for factorised noise, {"l1": (eps_w [F, H], eps_b [H]), "l2": (eps_w [H, A], eps_b [A])} for independent noise; None draws from
torch's generator in the reference's order."""
import torch
import torch.nn.functional as F

from jorldy_amd.core import network as P

from .networks import encode


def noisy_l(x, mu_w, sig_w, mu_b, sig_b, noise_type, is_train, draws=None):
    """utils.py:55-86 with injectable draws."""
    if not is_train:
        return torch.matmul(x, mu_w) + mu_b
    if noise_type == "factorized":
        if draws is not None:
            e_i, e_j = draws
        else:
            e_i = torch.randn(mu_w.size(0)).to(x.dtype)
            e_j = torch.randn(mu_b.size(0)).to(x.dtype)
        f_i = torch.sign(e_i) * torch.sqrt(torch.abs(e_i))
        f_j = torch.sign(e_j) * torch.sqrt(torch.abs(e_j))
        eps_w, eps_b = torch.matmul(f_i.unsqueeze(1), f_j.unsqueeze(0)), f_j
    else:
        if draws is not None:
            eps_w, eps_b = draws
        else:
            eps_w = torch.randn(mu_w.size()).to(x.dtype)
            eps_b = torch.randn(mu_b.size()).to(x.dtype)
    return torch.matmul(x, mu_w + sig_w * eps_w) + (mu_b + sig_b * eps_b)


class Noisy(P.Noisy):
    def forward(self, x, is_train, noise=None):
        x = encode(self.head, x)
        x = F.relu(noisy_l(x, self.mu_w1, self.sig_w1, self.mu_b1, self.sig_b1, self.noise_type, is_train, None if noise is None else noise["l1"]))
        return noisy_l(x, self.mu_w2, self.sig_w2, self.mu_b2, self.sig_b2, self.noise_type, is_train, None if noise is None else noise["l2"])

    def get_sig_w_mean(self):
        return torch.abs(self.sig_w1).mean(), torch.abs(self.sig_w2).mean()


def noise_dicts(noise, F_in, H, A, noise_type, dtype):
    """[sets, noise_len] flat noise sets in the library's format (= the reference's draw order) -> one `noise` dict per set."""
    out = []
    for s in range(noise.shape[0]):
        e, o, d = noise[s].to(dtype), 0, {}
        for tag, n_in, n_out in (("l1", F_in, H), ("l2", H, A)):
            if noise_type == "factorized":
                d[tag] = (e[o : o + n_in], e[o + n_in : o + n_in + n_out])
                o += n_in + n_out
            else:
                d[tag] = (e[o : o + n_in * n_out].view(n_in, n_out), e[o + n_in * n_out : o + n_in * n_out + n_out])
                o += n_in * n_out + n_out
        assert o == noise.shape[1]
        out.append(d)
    return out
