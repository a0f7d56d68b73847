"""The plumbing the network objects share below their architecture (csrc/jh_netcore.*, ops._NetObject), on every object that embeds it and
at the smallest shapes that take every branch of each layout (the shapes of test_abi_cpu.py's parameter-count test), max_batch 2:
the segment table, export_state -> import_state between two objects, and a refused create followed by a good one."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

S, H, MAXB, DEV = 3, 8, 2, "cuda:0"


def _rainbow(kind, head="mlp", hidden=H):
    from jorldy_amd import ops

    noise = "independent" if kind == "rainbow3" else "factorized"
    kind = "rainbow" if kind == "rainbow3" else kind
    return ops.RainbowNet((1, 36, 36) if head == "cnn" else S, 2, 3 if kind == "rainbow" else 1, hidden, head, MAXB, DEV, kind=kind, noise_type=noise)


def _iqn(hidden=H):
    from jorldy_amd import ops

    return ops.IQNNet(S, 3, 5, 2, hidden, MAXB, DEV)


def _ac(nc, hidden=H):
    from jorldy_amd import ops

    return ops.ACNet(S, 1, hidden, nc, MAXB, DEV)


def _sac(hidden=H):
    from jorldy_amd import ops

    return ops.SACNet(S, 1, hidden, MAXB, DEV)


MAKERS = {
    "rainbow-mlp": lambda **kw: _rainbow("rainbow", **kw), "dueling-mlp": lambda **kw: _rainbow("dueling", **kw), "q-mlp": lambda **kw: _rainbow("q", **kw),
    "rainbow-independent-mlp": lambda **kw: _rainbow("rainbow3", **kw), "rainbow-cnn": lambda **kw: _rainbow("rainbow", head="cnn", **kw),
    "iqn": _iqn, "acnet-1": lambda **kw: _ac(1, **kw), "acnet-2": lambda **kw: _ac(2, **kw), "sacnet": _sac,
}


def _ranges(net):
    """[(segment table, flat parameter bucket it indexes, name of the network for export / import or None)]"""
    if hasattr(net, "seg"):
        return [(net.seg, net.params, None)]
    return [(net.aseg, net.actor["params"], "actor")] + [(net.cseg, net.flat(f"critic{c + 1}"), f"critic{c + 1}") for c in range(net.nc)]


def _covered(seg, n):
    mask = torch.zeros(n, dtype=torch.bool)
    for off, rows, cols in seg.values():
        mask[off : off + rows * cols] = True
    return mask


def _packed(seg):
    """The table as the library packs it.  SACNet reports mu and log_std as four tensors in the reference's state_dict order, but keeps them
    as ONE [2A][H] layer and ONE [2A] bias (include/jorldy_hip.h: one contraction serves both): log_std's halves start A * H and A floats
    into those, wherever that falls.  The halves must tile the two packed segments exactly; the packing rules then apply to the whole."""
    if "log_std.weight" not in seg:
        return seg
    out = {k: v for k, v in seg.items() if not k.startswith(("mu.", "log_std."))}
    for kind in ("weight", "bias"):
        (o0, r0, c0), (o1, r1, c1) = seg["mu." + kind], seg["log_std." + kind]
        assert o1 == o0 + r0 * c0 and (r1, c1) == (r0, c0), kind
        out["mu|log_std." + kind] = (o0, r0 + r1, c0) if kind == "weight" else (o0, 1, c0 + c1)
    return out


@pytest.mark.parametrize("name", list(MAKERS))
def test_segment_table_is_sorted_aligned_disjoint_and_fills_the_bucket(name):
    net = MAKERS[name]()
    for seg, flat, _ in _ranges(net):
        seg, end = _packed(seg), 0
        for key, (off, rows, cols) in seg.items():  # table order
            assert off % 4 == 0, key
            assert off >= end, f"{key} starts at {off}, inside or in front of its predecessor (ends at {end})"
            end = off + rows * cols
        assert (end + 3) // 4 * 4 == flat.numel()
        assert any(rows * cols % 4 for _, rows, cols in seg.values()), "the shape leaves the padding nothing to do"


@pytest.mark.parametrize("name", list(MAKERS))
def test_export_then_import_into_a_fresh_object_copies_every_covered_word_and_no_padding(name):
    a, b = MAKERS[name](), MAKERS[name]()
    for (seg, flat_a, which), (_, flat_b, _) in zip(_ranges(a), _ranges(b)):
        n = flat_a.numel()
        flat_a.copy_(torch.arange(1, n + 1, dtype=torch.float32))  # exact in float32: n < 2^24
        args = () if which is None else (which,)
        b.import_state(a.export_state(*args), *args)
        mask = _covered(seg, n)
        got, want = flat_b.cpu(), flat_a.cpu()
        assert torch.equal(got[mask], want[mask])
        assert mask.sum() < n and not got[~mask].any(), "padding words were written"


def _forward(net):
    if hasattr(net, "seg") and net.cnn:
        out = net.forward(torch.zeros(MAXB, 1, 36, 36, dtype=torch.uint8, device=DEV))
    elif hasattr(net, "seg"):
        out = net.forward(torch.zeros(MAXB, S, device=DEV))
    else:
        x = torch.zeros(MAXB, S, device=DEV)
        out = net.actor_forward(x)
        out = net.critic_forward(x, torch.zeros(MAXB, net.A, device=DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(MAKERS))
def test_refused_create_is_an_argument_error_and_the_next_create_works(name):
    from jorldy_amd import _lib

    with pytest.raises(_lib.JhError, match="error -2"):  # JH_ERR_ARG: hidden 6 is no multiple of 4
        MAKERS[name](hidden=6)
    net = MAKERS[name]()
    out = _forward(net)
    assert torch.isfinite(out).all()


def test_create_entries_refuse_a_bad_size_themselves_and_hand_out_no_object():
    """The constructors above stop at the host-only *_param_count(s)_for entry; this is the create entry's own failure path."""
    from jorldy_amd import _lib

    lib, ctx = _lib.load(), _lib.ctx(0)
    b = [torch.zeros(16, device=DEV) for _ in range(10)]
    p = [_lib.ptr(t) for t in b]
    for call in (lambda h: lib.jh_rbnet_create(ctx, 0, 0, S, 0, 0, 6, 2, 3, MAXB, *p[:5], C.byref(h)),
                 lambda h: lib.jh_iqnnet_create(ctx, S, 6, 5, 2, 3, MAXB, *p[:5], C.byref(h)),
                 lambda h: lib.jh_acnet_create(ctx, S, 6, 1, 2, MAXB, *p, C.byref(h)),
                 lambda h: lib.jh_sacnet_create(ctx, S, 6, 1, MAXB, *p[:9], C.byref(h))):
        h = C.c_void_p()
        assert call(h) == -2 and not h.value
        assert b"bad argument" in lib.jh_last_error()
    assert torch.isfinite(_forward(_iqn())).all()
