"""LDMSAdaINRPNet (`network: ld_adain`) training on the GPU: the 7x7 conv's weight gradient
(rpst_conv7_wgrad) and data gradient (rpst_conv7 on flipped weights + rpst_reflect_pad_backward)
against float64 autograd, _stack_backward over a 7x7 Conv2dBlock, the whole step
(rpst.autograd.ld_losses) against the reference's recorded gradients (tests/golden/grads_ld*.npz,
gen_golden_ld_train.py) and against float64 CPU autograd of a restatement
(tests/ld_train_ref.py), determinism, the train.py driver, and what stays as it was.

Bars: kernels max(1e-5, 3 x floor), floor = the rel-L2 of torch's CPU fp32 autograd gradient of
the same inputs from float64 autograd (tests/test_gpu_ld.py's rule); network gradients
max(1e-4, 3 x floor) per tensor with the reference's floor read from the golden, or the
restatement's own fp32 distance (_floor_bars' rule)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import ld_ref as L
import ld_train_ref as LT
from helpers import gen, rel_l2, state_dict_of, synth_

pytestmark = pytest.mark.gpu

REFLECT, ZERO = 1, 0
MODE = {REFLECT: "reflect", ZERO: "constant"}

# (N, Cin, H, W, Cout), pad modes
WGRAD_CASES = [
    ((1, 8, 4, 4, 8), (REFLECT, ZERO)),        # reflect minimum: the mirrors overlap
    ((2, 5, 6, 5, 7), (REFLECT, ZERO)),        # channels not multiples of 8
    ((1, 20, 17, 33, 24), (REFLECT, ZERO)),    # ragged
    ((3, 32, 13, 9, 32), (REFLECT, ZERO)),     # odd batch
    ((1, 16, 9, 35, 16), (REFLECT, ZERO)),
    ((1, 40, 33, 70, 72), (REFLECT, ZERO)),    # crosses channel tiles and column segments
    ((2, 64, 24, 40, 64), (REFLECT, ZERO)),
    ((1, 16, 5, 130, 16), (REFLECT, ZERO)),    # wide row
    ((2, 128, 8, 12, 128), (REFLECT, ZERO)),
    ((1, 256, 8, 12, 256), (REFLECT, ZERO)),
    ((1, 8, 1, 1, 8), (ZERO,)),
    ((1, 8, 2, 3, 8), (ZERO,)),
]
DGRAD_CASES = WGRAD_CASES + [((1, 8, 4, 6, 8), (REFLECT,)), ((2, 12, 5, 4, 8), (REFLECT,)),
                             ((1, 8, 6, 5, 8), (REFLECT,))]


def _inputs(shape):
    n, cin, h, w, cout = shape
    x = gen(11, (n, cin, h, w), 1.0, 0.25)
    wt = gen(12, (cout, cin, 7, 7), (3.0 / (cin * 49)) ** 0.5)
    b = gen(13, (cout,), 0.5)
    dy = gen(14, (n, cout, h, w), 1.0, 0.1)
    return x, wt, b, dy


_REF = {}


def _ref_grads(shape, pad):
    """{dtype: (dx, dw, db)} of F.conv2d(F.pad(x, 3, mode)) by CPU autograd, computed once."""
    if (shape, pad) not in _REF:
        x, wt, b, dy = _inputs(shape)
        res = {}
        for dt in (torch.float32, torch.float64):
            xd, wd, bd = (t.detach().clone().to(dt).requires_grad_() for t in (x, wt, b))
            L.conv_pad(xd, wd, bd, MODE[pad]).backward(dy.to(dt))
            res[dt] = (xd.grad, wd.grad, bd.grad)
        _REF[(shape, pad)] = res
    return _REF[(shape, pad)]


def _bar(a32, a64):
    floor = rel_l2(a32, a64)
    return max(1e-5, 3 * floor), floor


def _conv(cuda, cin, cout, wt, b):
    conv = torch.nn.Conv2d(cin, cout, 7, bias=b is not None)
    with torch.no_grad():
        conv.weight.copy_(wt)
        if b is not None:
            conv.bias.copy_(b)
    return conv.to(cuda)


# ---- the kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("shape,pads", WGRAD_CASES, ids=[str(c[0]) for c in WGRAD_CASES])
def test_conv7_wgrad_vs_float64(cuda, shape, pads):
    from rpst import autograd as A
    n, cin, h, w, cout = shape
    x, wt, b, dy = _inputs(shape)
    conv = _conv(cuda, cin, cout, wt, b)
    for pad in pads:
        ref = _ref_grads(shape, pad)
        with torch.no_grad():
            dw, db = A.conv_wgrad7(x.to(cuda), dy.to(cuda), conv, pad)
        assert tuple(dw.shape) == (cout, cin, 7, 7) and tuple(db.shape) == (cout,)
        for name, got, k in (("dw", dw, 1), ("db", db, 2)):
            bar, floor = _bar(ref[torch.float32][k], ref[torch.float64][k])
            err = rel_l2(got, ref[torch.float64][k])
            print(f"wgrad7 {shape} pad {pad} {name}: rel-L2 {err:.3e}  bar max(1e-5, 3 x "
                  f"{floor:.3e}) = {bar:.3e}")
            assert err < bar, (shape, pad, name, err, bar)


def test_conv7_wgrad_deterministic_without_bias_and_checked(cuda):
    from rpst import _lib
    from rpst import autograd as A
    shape = (2, 40, 33, 70, 72)
    x, wt, b, dy = _inputs(shape)
    conv = _conv(cuda, 40, 72, wt, b)
    xc, gc = x.to(cuda), dy.to(cuda)
    with torch.no_grad():
        dw, db = A.conv_wgrad7(xc, gc, conv, REFLECT)
        dw2, db2 = A.conv_wgrad7(xc, gc, conv, REFLECT)
        assert torch.equal(dw, dw2) and torch.equal(db, db2)
        nob = _conv(cuda, 40, 72, wt, None)
        dw3, db3 = A.conv_wgrad7(xc, gc, nob, REFLECT)
        assert db3 is None and torch.equal(dw3, dw)
        x3, _, _, dy3 = _inputs((1, 8, 3, 8, 8))
        with pytest.raises(_lib.RpstError, match="reflect"):
            A.conv_wgrad7(x3.to(cuda), dy3.to(cuda), _conv(cuda, 8, 8, wt[:8, :8], None), REFLECT)


@pytest.mark.parametrize("shape,pads", DGRAD_CASES, ids=[str(c[0]) for c in DGRAD_CASES])
def test_conv7_dgrad_vs_float64(cuda, shape, pads):
    from rpst import autograd as A
    from rpst import ops, plan
    n, cin, h, w, cout = shape
    x, wt, b, dy = _inputs(shape)
    conv = _conv(cuda, cin, cout, wt, b)
    for pad in pads:
        ref = _ref_grads(shape, pad)
        step = plan.ConvStep(conv=conv, pad=pad, in_op=ops.IN_NONE, relu=ops.ACT_NONE)
        with torch.no_grad():
            dx = A.conv_dgrad(dy.to(cuda), step)
        assert tuple(dx.shape) == (n, cin, h, w)
        bar, floor = _bar(ref[torch.float32][0], ref[torch.float64][0])
        err = rel_l2(dx, ref[torch.float64][0])
        print(f"dgrad7 {shape} pad {pad}: rel-L2 {err:.3e}  bar max(1e-5, 3 x {floor:.3e}) = "
              f"{bar:.3e}")
        assert err < bar, (shape, pad, err, bar)


@pytest.mark.parametrize("pad_type", ["reflect", "zero"])
def test_stack_backward_7x7_block(cuda, pad_type):
    """_stack_backward over a compiled Conv2dBlock(16, 16, 7, 1, 3, inception_num=1) at 9 x 35
    against float64 autograd of the block: every parameter and the input gradient."""
    import network as net
    from rpst import autograd as A
    from rpst import plan
    blk = net.Conv2dBlock(16, 16, 7, 1, 3, inception_num=1, pad_type=pad_type)
    synth_(blk, 21)
    sd = state_dict_of(blk)
    x = gen(22, (2, 16, 9, 35), 1.0, 0.1)
    g = gen(23, (2, 16, 9, 35))

    def cpu_grads(dt):
        p = {k: v.detach().clone().to(dt).requires_grad_() for k, v in sd.items()}
        xd = x.detach().clone().to(dt).requires_grad_()
        L.block(xd, p, "", "reflect" if pad_type == "reflect" else "constant").backward(g.to(dt))
        return dict({k: v.grad for k, v in p.items()}, input=xd.grad)

    g64 = cpu_grads(torch.float64)
    g32 = cpu_grads(torch.float32)
    bars = {k: max(1e-5, 3 * rel_l2(g32[k], g64[k])) for k in g64}
    blk = blk.to(cuda)
    steps = plan.compile_layers(plan.block_layers(blk))
    assert [s.conv.kernel_size[0] for s in steps] == [7, 1]
    with torch.no_grad():
        _, saved = A._run_steps_saving(steps, x.to(cuda))
        grads = {}
        dx = A._stack_backward(steps, saved, g.to(cuda), grads, need_input_grad=True)
    named = dict(blk.named_parameters())
    assert sorted(named) == sorted(k for k in g64 if k != "input")
    got = dict({k: grads[id(p)] for k, p in named.items()}, input=dx)
    for k, gref in g64.items():
        err = rel_l2(got[k], gref)
        print(f"stack backward 7x7 {pad_type} {k}: {err:.3e} (bar {bars[k]:.3e})")
        assert err < bars[k], (k, err, bars[k])


# ---- the network --------------------------------------------------------------------------
def _net(cfg, seed, cuda):
    import network as net
    m = net.LDMSAdaINRPNet(cfg, copy.deepcopy(net.vgg))
    ck = synth_(m, seed)
    return m.to(cuda), ck


def _rp_names(m):
    return sorted(k for k, p in m.named_parameters() if p.requires_grad)


@pytest.mark.parametrize("i", range(len(LT.CASES)))
def test_ld_training_gradients_match_reference(cuda, golden, i):
    """ld_losses + total_loss.backward() against the reference's LDMSAdaINRPNet.forward +
    backward(): its fp32 losses at rtol 1e-5, every gradient tensor against its float64
    gradient within max(1e-4, 3 x the reference's own fp32 floor)."""
    from rpst import autograd as A
    g = golden("grads_ld")
    m, ck = _net(LT.golden_config(g, i), int(g[f"seed{i}"]), cuda)
    assert np.array_equal(ck, g[f"checksum{i}"])
    m.zero_grad()
    losses, total = A.ld_losses(m, torch.from_numpy(g[f"content{i}"]).to(cuda),
                                torch.from_numpy(g[f"style{i}"]).to(cuda))
    total.backward()
    assert set(losses) == {"style_loss", "content_loss", "total_loss"}
    for k in losses:
        assert rel_l2(losses[k].detach(), g[f"{k}{i}"]) < 1e-5, (i, k)
    named = dict(m.named_parameters())
    names = [str(n) for n in g[f"names{i}"]]
    assert sorted(names) == _rp_names(m)
    assert all(n.startswith(("rp_enc", "rp_dec")) for n in names)
    worst = 0.0
    for name in names:
        bar = max(1e-4, 3.0 * float(g[f"floor{i}:{name}"]))
        e = rel_l2(named[name].grad, g[f"grad64_{i}:{name}"])
        worst = max(worst, e / bar)
        assert e < bar, (i, name, e, bar)
        assert rel_l2(named[name].grad, g[f"grad{i}:{name}"]) < bar, (i, name, "fp32 golden")
    for name, p in named.items():
        if name.startswith("enc_"):
            assert p.grad is None, name
    print(f"ld reference gradients case {i}: worst err / bar {worst:.3e}")


@pytest.mark.parametrize("hidden,layers,inc,shape", [(4, 3, 0, (1, 3, 19, 37)),
                                                     (8, 3, 1, (2, 3, 16, 24))])
def test_ld_training_matches_cpu_autograd(cuda, hidden, layers, inc, shape):
    """Every gradient against float64 CPU autograd of the restatement (ld_train_ref) on ragged
    sizes, per tensor rel-L2 max(1e-4, 3 x the restatement's own fp32 distance)."""
    from rpst import autograd as A
    from rpst import synth
    m, _ = _net(LT.config(hidden, layers, inc), 97, cuda)
    sd = state_dict_of(m)
    c = torch.from_numpy(synth.image(9301, shape))
    s = torch.from_numpy(synth.image(9302, shape))
    ref_losses, g64 = LT.grads(c.double(), s.double(), sd, layers, 1.0, 10.0)
    _, g32 = LT.grads(c, s, sd, layers, 1.0, 10.0)
    bars = {k: max(1e-4, 3.0 * rel_l2(g32[k], g64[k])) for k in g64}
    m.zero_grad()
    losses, total = A.ld_losses(m, c.to(cuda), s.to(cuda))
    total.backward()
    for k in ("style_loss", "content_loss", "total_loss"):
        assert rel_l2(losses[k].detach(), ref_losses[k]) < 1e-5, k
    named = dict(m.named_parameters())
    assert sorted(g64) == _rp_names(m)
    worst = 0.0
    for name, gref in g64.items():
        e = rel_l2(named[name].grad, gref)
        worst = max(worst, e / bars[name])
        assert e < bars[name], (name, e, bars[name])
    print(f"ld cpu-autograd gradients {hidden}x{layers} inc {inc} {shape}: worst err / bar "
          f"{worst:.3e}")


def test_ld_training_deterministic_and_descends(cuda):
    """A repeated backward gives bit-identical gradients; five Adam steps lower total_loss."""
    from rpst import autograd as A
    from rpst import synth
    m, _ = _net(LT.config(4, 3, 1), 98, cuda)
    c = torch.from_numpy(synth.image(9303, (2, 3, 32, 32))).to(cuda)
    s = torch.from_numpy(synth.image(9304, (2, 3, 32, 32))).to(cuda)
    gs = []
    for _ in range(2):
        m.zero_grad()
        A.ld_losses(m, c, s)[1].backward()
        gs.append([p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(gs[0]) == sum(1 for p in m.parameters() if p.requires_grad)
    assert all(torch.equal(a, b) for a, b in zip(*gs))
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-4)
    totals = []
    for _ in range(5):
        opt.zero_grad()
        _, total = A.ld_losses(m, c, s)
        total.backward()
        opt.step()
        totals.append(float(total.detach()))
    assert totals[-1] < totals[0], totals


def test_ld_train_driver_end_to_end(cuda, tmp_path):
    """train.py with `network: ld_adain`: logs every iteration, stylises the test pair at
    test_iter, writes the whole state_dict as its checkpoint; a fresh model resumes from it."""
    import yaml
    from PIL import Image

    import network as net
    import train as train_driver
    rng = np.random.default_rng(3)
    for d in ("content", "style/a", "test/content", "test/style"):
        os.makedirs(tmp_path / d)
    for k in range(3):
        for d in ("content", "style/a"):
            Image.fromarray(rng.integers(0, 256, (40, 48, 3), dtype=np.uint8)).save(
                tmp_path / d / f"{k}.png")
    for d in ("test/content", "test/style"):
        Image.fromarray(rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(
            tmp_path / d / "t.png")
    cfg = dict(LT.config(4, 3), network="ld_adain", vgg="unused", lr=1e-4, lr_decay=5e-5,
               max_iter=5, batch_size=2, num_workers=2, img_size=32,
               content_dir=str(tmp_path / "content"), style_dir=str(tmp_path / "style"),
               test_dir=str(tmp_path / "test"), test_dataset="paired", test_iter=2, log_iter=1,
               snapshot_save_iter=2, output=str(tmp_path / "out"))
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    assert train_driver.main(["--config", str(path), "--synthetic-weights", "3"]) == 0
    lines = [json.loads(ln) for ln in open(tmp_path / "out" / "logs" / "train.jsonl")]
    assert [ln["iteration"] for ln in lines] == [1, 2, 3, 4]
    assert all(np.isfinite(ln["total_loss"]) for ln in lines)
    assert (tmp_path / "out" / "test" / "2" / "t-t.png").exists()
    assert (tmp_path / "out" / "test" / "4" / "t-t-cat.png").exists()
    ck_path = tmp_path / "out" / "checkpoints" / "4"
    ck = torch.load(ck_path, weights_only=True, map_location="cpu")
    m2 = net.LDMSAdaINRPNet(dict(cfg, resume=True, checkpoint_path=str(ck_path)),
                            copy.deepcopy(net.vgg)).to(cuda)
    assert m2.begin == 4
    assert set(ck) == set(m2.state_dict())
    assert "rp_enc1_big_revf.conv.weight" in ck and "enc_1.0.weight" in ck
    for k, v in m2.state_dict().items():
        assert torch.equal(v.cpu(), ck[k]), k
    # the checkpoint holds trained weights, not the initial ones
    import stylize
    m0 = stylize.build_network(cfg, synthetic_seed=3)
    assert not torch.equal(m0.state_dict()["rp_enc1_big_revf.conv.weight"],
                           ck["rp_enc1_big_revf.conv.weight"])


# ---- unchanged surface --------------------------------------------------------------------
def test_forward_still_raises_and_no_cpu_fallback(cuda):
    """(Name kept.) forward() with autograd enabled trains: m(c, s)[1].backward() leaves on every
    rp_enc* / rp_dec* parameter the gradient of ld_losses(...)[1].backward() on a copy of the
    model, bit for bit; ld_losses still refuses CPU tensors."""
    from rpst import autograd as A
    from rpst import synth
    m, _ = _net(LT.config(4, 3, 0), 99, cuda)
    m2 = copy.deepcopy(m)
    c = torch.from_numpy(synth.image(9305, (1, 3, 16, 24))).to(cuda)
    s = torch.from_numpy(synth.image(9306, (1, 3, 16, 24))).to(cuda)
    m(c, s)[1].backward()
    A.ld_losses(m2, c, s)[1].backward()
    named, named2 = dict(m.named_parameters()), dict(m2.named_parameters())
    names = [k for k in named if k.startswith(("rp_enc", "rp_dec"))]
    assert sorted(names) == _rp_names(m) and len(names) == 2 * (2 * 3 + 3)
    for k in names:
        assert named[k].grad is not None and bool(torch.isfinite(named[k].grad).all()), k
        assert torch.equal(named[k].grad, named2[k].grad), k
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        A.ld_losses(m, c.cpu(), c.cpu())
