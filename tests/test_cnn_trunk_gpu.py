"""The convolutional trunk of the native value networks (jh_rbnet_*: conv1 on the dedicated kernels or on the tile engine's NCHW operands,
conv2 / conv3 as implicit GEMMs) against FLOAT64 ground truth at every frame layout and dispatch edge of its first layer -- the legs
that the Atari layout of tests/test_rbnet_gpu.py (uint8, 4 planes, W % 4 == 0, (H - 8) % 4 == (W - 8) % 4 == 0) never takes.

Truth and criterion are those of tests/test_rbnet_gpu.py, unchanged: the reference's module (tests/mirror: discrete_q_network, and
discrete_policy_value for PPO's entry) on the CPU in float64 with de-symmetrised fp32-representable parameters, torch-CPU float32 beside it,
    |ours - fp64| / max|fp64| <= max(1e-5, 2 x |torch_fp32 - fp64| / max|fp64|)      per tensor (tests/fp64_truth.py: vs_exact)
on the three outputs of learn_forward, on every parameter gradient after backward and on an eval forward of one row.  No row or element is
left out of any comparison; no GPU library is a comparator.  kind "q", hidden 32, 3 actions: the cases are about the trunk.

B is learn_forward's batch: the online net sees 2B frames and the target net B frames in one grouped launch per layer.  P1 = conv1's
output pixels per frame, K = 64 Cin = conv1's reduction length.

  id               state       frames  B    the leg of conv1 it pins
  rgb_procgen      (3,64,64)   u8      5    forward: tile engine, NCHW_K packed uint8 (one dword = 4 taps), Cin % 4 != 0; wgrad: NCHW_X uint8
  gray_min         (1,36,36)   u8      3    K = 64 (two chunks), smallest legal image: conv3's output is 1 x 1 (P3 = 1, F = 64)
  odd_width        (4,45,50)   u8      4    W % 4 != 0: element-wise uint8 fetch both ways; floor in OH and OW (a row and two columns unused)
  f32_vec          (4,44,52)   f32     4    fp32 frames 0..255 (true division by 255), forward AND backward (last_x_u8 == 0); then the same frames as uint8
  f32_odd          (3,45,50)   f32     3    fp32 frames with fractional values, unaligned rows, Cin = 3
  c8_two_rounds    (8,44,52)   u8      3    forward on the tile engine, dedicated wgrad kernel with 2 channel rounds (P1 = 120)
  c20_table_split  (20,36,40)  u8      2    K = 1280 > the LDS offset table (1024), under the heuristic's own 10-way split of 5 / 3 / 2 tiles (128 k's each: the table's
                                            floor of 2 splits does not bind here); dedicated wgrad, 5 rounds (P1 = 72), and the ONLY small case of its single-group tail
                                            loop: 36 groups, the second workgroup's slices hold 5, 5, 5 and 1, and a slice crosses the frame boundary at group 18
  c20_table_clamp  (20,36,40)  u8      128  the same K where the heuristic asks for ONE split: 288 and 144 tiles of 64 rows (>= 128 each: no split to fill the chip, and
                                            the launch-time model keeps the multiplier 1), so the floor ceil(1280 / 1024) = 2 is what keeps a split's 640 k's inside
                                            the table (B = 58, the first with >= 128 online tiles, does not do: the model picks the multiplier 2 there).  With the
                                            floor replaced by an error return in jh_tgemm_launch this case alone fails; dedicated wgrad over 2304 groups
                                            (116 workgroups, a tail of 4 single groups)
  c12_p_odd        (12,44,48)  u8      3    Cin % 4 == 0 but P1 = 110: wgrad on the tile engine, K = 768
  ragged_66        (4,44,48)   u8      22   dedicated forward kernel, 7 tiles of 16 pixels (the last holds 14), 66 frames: bracket 64-191
  ragged_192       (4,44,48)   u8      64   ... 192 frames: bracket 192-511
  ragged_513       (4,44,48)   u8      171  ... 513 frames: bracket >= 512; tile-engine wgrad over 18 810 pixels
  wgrad_parts_1    (4,44,52)   u8      1    dedicated wgrad: 30 pixel groups on 2 workgroups of 4 slices x 5 groups: the second one's slices hold 5, 5, 0 and 0 (empty slices
                                            add zeros).  30 B groups are always whole rounds of 5: at this shape no slice holds 1-4 groups (c20_table_split has that)
  wgrad_parts_171  (4,44,52)   u8      171  dedicated wgrad: 5130 groups over 128 workgroups of 40 + a last one of 10

plus rgb_procgen through kind "pv" (15 actions + the value row; forward_keep -> backward: PPO's entry, one job per launch) against
discrete_policy_value, and the construction limits (35 x 40 refused, (20, 36, 40) accepted with the float64 module's parameter count).

What the reference costs (e_ref = |torch_fp32 - fp64| / max|fp64|, the worst tensor of its group, CPU) and what we cost (e_ours, MI355X); the
allowance of a tensor is max(1e-5, 2 e_ref):

  id               e_ref outputs  e_ref grads   e_ours outputs  e_ours grads
  rgb_procgen      6.3e-07        4.2e-07       1.1e-06         3.9e-07
  gray_min         4.7e-07        4.3e-07       4.1e-07         5.2e-07
  odd_width        6.9e-07        5.3e-07       7.2e-07         3.6e-07
  f32_vec          1.6e-06        5.9e-07       5.1e-07         5.5e-07
   ... as uint8    1.6e-06        5.9e-07       8.4e-07         7.4e-07
  f32_odd          4.8e-07        6.2e-07       4.9e-07         8.0e-07
  c8_two_rounds    1.5e-06        9.0e-07       9.4e-07         5.2e-07
  c20_table_split  3.0e-06        1.5e-06       1.3e-06         7.6e-07
  c20_table_clamp  1.6e-06        1.5e-06       1.3e-06         9.6e-07
  c12_p_odd        5.9e-07        6.7e-07       3.2e-07         4.2e-07
  ragged_66        1.2e-06        1.0e-06       1.2e-06         5.9e-07
  ragged_192       1.4e-06        1.7e-06       1.3e-06         6.6e-07
  ragged_513       1.3e-06        5.8e-06       1.3e-06         7.4e-07
  wgrad_parts_1    7.8e-07        5.1e-07       6.4e-07         5.3e-07
  wgrad_parts_171  1.3e-06        3.0e-06       8.6e-07         6.7e-07
  rgb_procgen pv   1.6e-06        3.7e-07       7.3e-07         4.5e-07

2 e_ref stays below the floor everywhere but in ragged_513's gradients (1.2e-5): the floor 1e-5 is the allowance, and we use at most 13 % of it.
The float64 side of the largest case takes under a second of CPU time.  The tests print e_ours (pytest -s).
"""
import pytest

import fp64_truth as T
from test_rbnet_gpu import _grads_vs_exact, _mk_kind, _net64

pytestmark = pytest.mark.gpu

TOL = 1e-5
H, A = 32, 3

# id -> (state, frames, B)
CASES = {
    "rgb_procgen": ((3, 64, 64), "u8", 5),
    "gray_min": ((1, 36, 36), "u8", 3),
    "odd_width": ((4, 45, 50), "u8", 4),
    "f32_vec": ((4, 44, 52), "f32_bytes", 4),
    "f32_odd": ((3, 45, 50), "f32", 3),
    "c8_two_rounds": ((8, 44, 52), "u8", 3),
    "c20_table_split": ((20, 36, 40), "u8", 2),
    "c20_table_clamp": ((20, 36, 40), "u8", 128),
    "c12_p_odd": ((12, 44, 48), "u8", 3),
    "ragged_66": ((4, 44, 48), "u8", 22),
    "ragged_192": ((4, 44, 48), "u8", 64),
    "ragged_513": ((4, 44, 48), "u8", 171),
    "wgrad_parts_1": ((4, 44, 52), "u8", 1),
    "wgrad_parts_171": ((4, 44, 52), "u8", 171),
}


def _frames(S, frames, rows, g):
    """-> CPU frames in the dtype the native net is given: uint8, fp32 holding byte values ("f32_bytes") or fp32 with fractional values in [0, 255)."""
    import torch

    if frames == "f32":
        return torch.rand((rows,) + tuple(S), generator=g) * 255.0
    x = torch.randint(0, 256, (rows,) + tuple(S), dtype=torch.uint8, generator=g)
    return x.float() if frames == "f32_bytes" else x


def _q_truth(nets, x, B, gl):
    """learn_forward -> backward -> eval forward of the target net on next_state's first row, in float64 and in torch-CPU float32.
    -> {name: (exact, ref32)} of the four outputs; the gradients are left in ref64 / ref32's .grad."""
    import torch

    (ref64, ref32), (tgt64, tgt32) = nets
    for m in (ref64, ref32):
        m.zero_grad()
    x64, x32 = x.double(), x.float()
    q0, q0_32 = ref64(x64[:B]), ref32(x32[:B])
    with torch.no_grad():
        out = {"online(state)": (q0.detach(), q0_32.detach()), "online(next_state)": (ref64(x64[B:]), ref32(x32[B:])),
               "target(next_state)": (tgt64(x64[B:]), tgt32(x32[B:])), "target eval forward, 1 row": (tgt64(x64[B : B + 1]), tgt32(x32[B : B + 1]))}
    q0.backward(gl.double())
    q0_32.backward(gl)
    return out


def _pv_truth(nets, x, gl):
    """forward_keep -> backward of the policy-value net: raw logits | value and d/d(parameters) of sum(gl * [logits | v])."""
    import torch

    out, n = {}, gl.shape[1] - 1
    for m, dt in zip(nets, (torch.float64, torch.float32)):
        m.zero_grad()
        logits, v = m.raw(x.to(dt))
        torch.autograd.backward([logits, v], [gl[:, :n].to(dt), gl[:, n:].to(dt)])
        out[dt] = (logits.detach(), v.detach())
    return {"logits": (out[torch.float64][0], out[torch.float32][0]), "value": (out[torch.float64][1], out[torch.float32][1])}


def _case_inputs(name):
    import torch

    S, frames, B = CASES[name]
    g = torch.Generator().manual_seed(1)
    return S, B, _frames(S, frames, 2 * B, g), torch.randn(B, A, generator=g) / B


def _run_q(nat, nets, x, B, gl, tag):
    """The native side of _q_truth on the frames `x` as they are (uint8 or fp32), every tensor against float64.  -> (worst e_ours of the outputs, of the gradients)."""
    import torch

    truth = _q_truth(nets, x, B, gl)
    x_dev = x.cuda()
    out = torch.empty(3, B, A, 1, device="cuda")
    nat.learn_forward(x_dev, B, None, out)
    e_out = [T.vs_exact(out[j, :, :, 0], *truth[k], TOL, f"{tag} {k}")[0] for j, k in enumerate(("online(state)", "online(next_state)", "target(next_state)"))]
    nat.backward(gl.cuda().contiguous())
    torch.cuda.synchronize()
    (ref64, ref32), _ = nets
    p32 = dict(ref32.named_parameters())
    grads = _grads_vs_exact(nat, ref64, ref32, tag=f"{tag} ")
    rel = lambda a, e: float((a.double().cpu().reshape(e.shape) - e).abs().max()) / (float(e.abs().max()) + 1e-30)
    e_grad = max(rel(grads[k], p.grad) for k, p in ref64.named_parameters())
    assert set(grads) == set(p32)
    got = nat.forward(x_dev[B : B + 1], which=1)
    k = "target eval forward, 1 row"
    e_out.append(T.vs_exact(got[:, :, 0], *truth[k], TOL, f"{tag} {k}")[0])
    return max(e_out), e_grad


@pytest.mark.parametrize("name", list(CASES))
def test_cnn_trunk_learn_forward_backward_and_eval_match_float64(name):
    S, B, x, gl = _case_inputs(name)
    (ref64, ref32), (tgt64, tgt32), nat = _mk_kind("q", "cnn", S, A, H, B)
    nets = ((ref64, ref32), (tgt64, tgt32))
    e = _run_q(nat, nets, x, B, gl, name)
    print(f"[cnn_trunk] {name}: e_ours outputs {e[0]:.1e} grads {e[1]:.1e}")
    if CASES[name][1] == "f32_bytes":  # the same frames as uint8: same fp32 operands (byte / 255 correctly rounded), the dedicated kernels' summation order
        import torch

        e = _run_q(nat, nets, x.to(torch.uint8), B, gl, name + " as uint8")
        print(f"[cnn_trunk] {name} as uint8: e_ours outputs {e[0]:.1e} grads {e[1]:.1e}")


def test_cnn_trunk_policy_value_rgb_procgen_matches_float64():
    """PPO's entry on config.ppo.procgen's frames: kind "pv" (15 actions + the value row in ONE last layer), forward_keep -> backward, one job per launch."""
    import torch
    from jorldy_amd import ops

    S, B, n_act = (3, 64, 64), 5, 15
    m64, m32 = _net64("discrete_policy_value", S, n_act, D_hidden=H, head="cnn")
    nat = ops.RainbowNet(S, n_act, 1, H, "cnn", B, "cuda:0", kind="pv")
    nat.import_state(m32.state_dict(), nat.params)
    assert list(nat.export_state().keys()) == list(m32.state_dict().keys())
    g = torch.Generator().manual_seed(2)
    x = _frames(S, "u8", B, g)
    gl = torch.randn(B, n_act + 1, generator=g) / B
    truth = _pv_truth((m64, m32), x, gl)
    heads = torch.empty(B, n_act + 1, device="cuda")
    x_dev = x.cuda()  # stays alive until after backward(): conv1's weight gradient re-reads the frames
    nat.forward_keep(x_dev, heads)
    e_l = T.vs_exact(heads[:, :n_act], *truth["logits"], TOL, "pv logits")[0]
    e_v = T.vs_exact(heads[:, n_act:], *truth["value"], TOL, "pv value")[0]
    nat.backward(gl.cuda().contiguous())
    torch.cuda.synchronize()
    grads = _grads_vs_exact(nat, m64, m32, tag="pv ")
    rel = lambda a, e: float((a.double().cpu().reshape(e.shape) - e).abs().max()) / (float(e.abs().max()) + 1e-30)
    print(f"[cnn_trunk] rgb_procgen pv: e_ours outputs {max(e_l, e_v):.1e} grads {max(rel(grads[k], p.grad) for k, p in m64.named_parameters()):.1e}")


def test_cnn_trunk_refuses_small_images_and_accepts_any_plane_count():
    """jh_rbnet_create asks c_or_s > 0 of the plane count and nothing more; an image below 36 x 36 (conv3 would have no output pixel) is refused at construction."""
    from jorldy_amd import ops
    from jorldy_amd._lib import JhError

    with pytest.raises(JhError, match="36x36"):
        ops.RainbowNet((4, 35, 40), A, 1, H, "cnn", 2, "cuda:0", kind="q")
    with pytest.raises(JhError, match="36x36"):
        ops.RainbowNet((4, 40, 35), A, 1, H, "cnn", 2, "cuda:0", kind="q")
    S = (20, 36, 40)
    for n_act in (4, A):  # the flat bucket starts every tensor at a multiple of 4 floats: 4 actions pack without a gap, 3 leave one float behind q.bias
        m64, _ = _net64("discrete_q_network", S, n_act, D_hidden=H, head="cnn")
        nat = ops.RainbowNet(S, n_act, 1, H, "cnn", 2, "cuda:0", kind="q")
        assert nat.n_params == sum((p.numel() + 3) // 4 * 4 for p in m64.parameters())
        if n_act == 4:
            assert nat.n_params == sum(p.numel() for p in m64.parameters())
        sd = nat.export_state()
        assert [(k, v.numel()) for k, v in sd.items()] == [(k, p.numel()) for k, p in m64.named_parameters()]
