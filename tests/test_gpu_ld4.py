"""LDMSAdaINRPNet4 (`network: ld_adain4`, reference network/adain_rp.py:711-819) on the GPU: the
three bandwidth kernels (rpst_resize_nearest bit for bit against torch's CPU F.interpolate,
rpst_resized_mean_std and rpst_ld4_fuse against float64), test() / encode_rp_intermediate
against the reference's recorded outputs (tests/golden/ld4*.npz, gen_golden_ld4.py), the fused
route against the op-by-op one, the launch sequence, save / resume and the stylize pipeline.

Bars: TOL_STATS (1e-5 rel-L2) for statistics and the AdaIN affine, TOL_NET / TOL_NET_MAXABS end
to end (tests/helpers.py), levels at max(1e-5, 3 x the reference's own fp32 distance to its
float64 run), as tests/test_gpu_ld.py holds its convs."""
import copy
import re

import pytest
import torch
import torch.nn.functional as F

import ld4_ref as L4
import ld_ref as L
from helpers import (TOL_NET, TOL_NET_MAXABS, TOL_STATS, check_pipeline, dataset_tree, dev, gen,
                     golden_net, mask_kw, max_abs_ratio, rel_l2, synth_, traced_launches,
                     unfused)

pytestmark = pytest.mark.gpu

SENTINEL = -12345.5


# ---- the kernels --------------------------------------------------------------------------
# (N, C, h, w) -> (H, W)
RESIZE_CASES = [
    ((1, 1, 1, 1), (1, 1)),
    ((1, 3, 1, 1), (5, 7)),
    ((2, 4, 3, 4), (5, 7)),
    ((1, 8, 9, 17), (17, 33)),
    ((1, 5, 2, 3), (19, 37)),
    ((2, 16, 16, 24), (32, 48)),
    ((1, 4, 4, 6), (32, 48)),
    ((1, 4, 6, 10), (6, 10)),
    ((1, 2, 3, 130), (5, 259)),
    # past one chunk of 4096 destination elements (write_plane_chunk's chunk > 0) and one
    # stride of 256 source quads (resized_stats_kernel):
    ((2, 5, 33, 34), (65, 67)),    # 4355 = 2 chunks, odd: the planes' heads cycle 0-3; the
                                   # source's 1122 = 2 strides and a 2-element tail
    ((1, 3, 23, 29), (65, 67)),    # non-integer ratios on both axes
    ((1, 2, 40, 52), (91, 93)),    # 8463 = 3 chunks; the source's 2080 = 3 strides
    ((1, 4, 64, 64), (128, 128)),  # 4 full chunks, aligned, exactly 2 x
]
RESIZE_IDS = [f"{s[0]}->{s[1]}" for s in RESIZE_CASES]


@pytest.mark.parametrize("shape,size", RESIZE_CASES, ids=RESIZE_IDS)
def test_resize_nearest_equals_torch(cuda, shape, size):
    from rpst import ops
    n, c = shape[:2]
    x = gen(41, shape, 2.0, 0.5)
    want = F.interpolate(x, size)
    got = ops.resize_nearest(x.to(cuda), size)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    # into the upper slice of a destination twice as wide: the lower slice is left alone
    out = torch.full((n, 2 * c, *size), SENTINEL, device=cuda)
    res = ops.resize_nearest(x.to(cuda), size, out=out, out_channel_offset=c)
    assert res is out
    assert torch.equal(out[:, c:].cpu(), want)
    assert torch.equal(out[:, :c], torch.full_like(out[:, :c], SENTINEL))


def test_resize_nearest_argument_checks(cuda):
    from rpst import _lib, ops
    x = torch.zeros((1, 4, 3, 4), device=cuda)
    with pytest.raises(ValueError, match="enlarges only"):
        ops.resize_nearest(x, (2, 7))
    with pytest.raises(ValueError, match="channel offset"):
        ops.resize_nearest(x, (5, 7), out_channel_offset=4)
    with pytest.raises(ValueError, match="out must"):
        ops.resize_nearest(x, (5, 7), out=torch.zeros((1, 4, 5, 8), device=cuda))
    with pytest.raises(_lib.RpstError, match="channels"):
        ops.resize_nearest(x, (5, 7), out=torch.zeros((1, 6, 5, 7), device=cuda),
                           out_channel_offset=4)


@pytest.mark.parametrize("shape,size", RESIZE_CASES, ids=RESIZE_IDS)
def test_resized_mean_std_vs_float64(cuda, shape, size):
    from rpst import ops
    x = gen(42, shape, 2.0, 0.5)
    mean, std = ops.resized_mean_std(x.to(cuda), size)
    assert tuple(mean.shape) == tuple(std.shape) == (*shape[:2], 1, 1)
    m2, s2 = ops.resized_mean_std(x.to(cuda), size)  # a second run: the same bits (NaN too)
    assert torch.equal(mean.view(torch.int32), m2.view(torch.int32))
    assert torch.equal(std.view(torch.int32), s2.view(torch.int32))
    if size == (1, 1):  # one element: the mean is it, the std NaN, as rpst_calc_mean_std gives
        assert torch.equal(mean.cpu(), x) and bool(torch.isnan(std).all())
        rm, rs = ops.calc_mean_std(x.to(cuda))
        assert torch.equal(mean, rm) and bool(torch.isnan(rs).all())
        return
    rm, rs = L.mean_std(F.interpolate(x, size).double())
    em, es = rel_l2(mean, rm), rel_l2(std, rs)
    print(f"resized_mean_std {shape} -> {size}: mean {em:.2e} std {es:.2e}")
    assert em < TOL_STATS and es < TOL_STATS


def test_resized_mean_std_survives_a_large_mean(cuda):
    """Values 100 +- 1: a one-pass uncentred second moment would lose the spread in fp32."""
    from rpst import ops
    x = gen(43, (2, 4, 9, 17), 1.0, 100.0)
    mean, std = ops.resized_mean_std(x.to(cuda), (17, 33))
    rm, rs = L.mean_std(F.interpolate(x, (17, 33)).double())
    assert rel_l2(mean, rm) < TOL_STATS and rel_l2(std, rs) < TOL_STATS


def _fuse_case(cuda, ca, hd, size, csize, n=2):
    """ld4_fuse on ld4_ref.fuse_inputs -> (y, the kernel's output, the float64 reference)."""
    from rpst import ops
    y, fine, coarse, stats = L4.fuse_inputs(ca, hd, size, csize, n)
    params = [ops.adain_params(*(t.to(cuda) for t in (s[0], s[1], s[2], s[3]))) for s in stats]
    got = ops.ld4_fuse(None if y is None else y.to(cuda), fine.to(cuda), coarse.to(cuda),
                       params[0], params[1], n=n)
    return y, got, L4.fuse_want(fine, coarse, stats, size, n)


@pytest.mark.parametrize("ca", [0, 4, 3])
@pytest.mark.parametrize("hd", [4, 5])
@pytest.mark.parametrize("size,csize", [((17, 33), (9, 17)), ((24, 40), (12, 20)),
                                        ((32, 48), (1, 2)), ((65, 67), (33, 34)),
                                        ((91, 93), (23, 29)), ((128, 128), (64, 64))])
def test_ld4_fuse_vs_float64(cuda, ca, hd, size, csize):
    y, got, want = _fuse_case(cuda, ca, hd, size, csize)
    assert tuple(got.shape) == (2, ca + 2 * hd, *size) and got.dtype == torch.float32
    if ca:
        assert torch.equal(got[:, :ca].cpu(), y)
    err = rel_l2(got[:, ca:], want)
    assert err < TOL_STATS, (ca, hd, size, csize, err)
    for k in range(2):  # per image too: image 1 does not ride on image 0's statistics
        assert rel_l2(got[k, ca:], want[k]) < TOL_STATS
    # and per destination chunk of 4096 elements of each plane: one wrong chunk of one plane
    # is not diluted by the rest
    hw = size[0] * size[1]
    g, w = got[:, ca:].cpu().double().reshape(-1, hw), want.reshape(-1, hw)
    worst = max(float((g[:, o:o + L4.CHUNK] - w[:, o:o + L4.CHUNK]).norm(dim=1)
                      .div(w[:, o:o + L4.CHUNK].norm(dim=1)).max())
                for o in range(0, hw, L4.CHUNK))
    if hw > L4.CHUNK:
        print(f"ld4_fuse {ca}+2x{hd} {csize}->{size}: rel-L2 {err:.3e}, worst chunk of a plane "
              f"{worst:.3e}")
    assert worst < TOL_STATS, (ca, hd, size, csize, worst)


def test_ld4_fuse_argument_checks(cuda):
    from rpst import ops
    fine, coarse = torch.zeros((2, 4, 5, 7), device=cuda), torch.zeros((2, 4, 3, 4), device=cuda)
    p = torch.ones(16, device=cuda)
    with pytest.raises(ValueError, match="params"):
        ops.ld4_fuse(None, fine, coarse, p, p)  # n = 2 needs 32
    with pytest.raises(ValueError, match="y must be"):
        ops.ld4_fuse(torch.zeros((1, 3, 5, 8), device=cuda), fine, coarse, p, p)
    with pytest.raises(ValueError, match="enlarges only"):
        ops.ld4_fuse(None, fine, torch.zeros((2, 4, 6, 4), device=cuda), p, p, n=1)
    with pytest.raises(ValueError, match="coarse"):
        ops.ld4_fuse(None, fine, torch.zeros((2, 5, 3, 4), device=cuda), p, p, n=1)
    assert tuple(ops.ld4_fuse(None, fine, coarse, p, p, n=1).shape) == (1, 8, 5, 7)


# ---- the network --------------------------------------------------------------------------
def _net(g, i, cuda):
    import network as net
    return golden_net(net.LDMSAdaINRPNet4, L4.golden_config(g, i), g, f"net{i}_", cuda)


@pytest.mark.parametrize("i", range(len(L4.CASES)))
def test_ld4_test_matches_reference(cuda, golden, i, tmp_path):
    import network.adain_rp as arp
    g = golden("ld4")
    m = _net(g, i, cuda)
    c, s = dev(g[f"net{i}_content"], cuda), dev(g[f"net{i}_style"], cuda)
    masked = bool(g[f"net{i}_use_mask"])
    kw = mask_kw(g, f"net{i}_", cuda, tmp_path if masked else None)  # the masks as files
    y = m.test(c, s, **kw)
    assert m.training  # test() leaves the model in training mode, as the reference does
    ref = g[f"net{i}_out"]
    err, mx = rel_l2(y, ref), max_abs_ratio(y, ref)
    print(f"ld4 case {i}: rel-L2 {err:.3e} max-abs ratio {mx:.3e} (reference floor "
          f"{float(g[f'net{i}_floor']):.2e})")
    assert err < TOL_NET and mx < TOL_NET_MAXABS
    assert torch.equal(y, m.test(c, s, **kw))  # a repeated test() is bit-identical
    if masked:  # and from label maps already at the image size
        yt = m.test(c, s, **mask_kw(g, f"net{i}_", cuda))
        assert rel_l2(yt, ref) < TOL_NET and max_abs_ratio(yt, ref) < TOL_NET_MAXABS
    with unfused(arp, "FUSED_ADAIN"):
        plain = m.test(c, s, **kw)
    assert rel_l2(plain, ref) < TOL_NET and max_abs_ratio(plain, ref) < TOL_NET_MAXABS
    assert rel_l2(y, plain) < TOL_NET
    m.eval()
    with torch.no_grad():
        dec = m.decode(m.encode_rp_intermediate(c), m.encode_rp_intermediate(s),
                       use_mask=masked, **kw)
    assert torch.equal(dec, plain)


@pytest.mark.parametrize("i", [i for i, cs in enumerate(L4.CASES)
                               if L4.level_bytes(cs[0], cs[1], cs[3]) < L4.LEVEL_BYTES])
def test_ld4_encoder_levels_match_reference(cuda, golden, i):
    g = golden("ld4")
    assert bool(g[f"net{i}_has_levels"])
    m = _net(g, i, cuda)
    with torch.no_grad():
        levels = m.encode_rp_intermediate(dev(g[f"net{i}_content"], cuda))
    assert len(levels) == int(g[f"net{i}_layers"])
    for k, lv in enumerate(levels):
        ref = g[f"net{i}_level{k}_64"]
        assert tuple(lv.shape) == tuple(ref.shape)
        floor = float(g[f"net{i}_level{k}_floor"])
        err, bar = rel_l2(lv, ref), max(1e-5, 3 * floor)
        print(f"ld4 case {i} level {k}: rel-L2 {err:.3e} bar max(1e-5, 3 x {floor:.2e})")
        assert err < bar, (i, k, err, bar)


def test_ld4_test_at_72x88_vs_float64(cuda):
    """test() at a size whose planes need two chunks (72 x 88 = 6336 elements; the coarse
    sources 36 x 44 = 1584 and 18 x 22 = 396 elements: two strides of the statistics loop and
    one), against the float64 restatement on the same weights: TOL_NET / TOL_NET_MAXABS, and
    held as the levels are, to max(1e-5, 3 x the fp32 restatement's own distance to float64)."""
    import network as net
    m = net.LDMSAdaINRPNet4(L4.config(4, 3, 0, 3), copy.deepcopy(net.vgg))
    synth_(m, 96)
    sd = m.state_dict()
    c, s = gen(61, (1, 3, 72, 88), 0.5, 0.5), gen(62, (1, 3, 72, 88), 0.5, 0.5)
    ref = L4.test(c, s, sd, 3)
    floor = rel_l2(L4.test(c, s, sd, 3, dtype=torch.float32), ref)
    assert ref.dtype == torch.float64 and floor < 3e-6
    m = m.to(cuda)
    y = m.test(c.to(cuda), s.to(cuda))
    err, mx, bar = rel_l2(y, ref), max_abs_ratio(y, ref), max(1e-5, 3 * floor)
    print(f"ld4 72x88: rel-L2 {err:.3e} max-abs ratio {mx:.3e} bar max(1e-5, 3 x {floor:.2e})")
    assert err < TOL_NET and mx < TOL_NET_MAXABS
    assert err < bar, (err, bar)


def test_ld4_batch_of_two_equals_single_images(cuda, golden):
    g = golden("ld4")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    y = m.test(c, s)
    for k in range(2):
        assert torch.equal(y[k:k + 1], m.test(c[k:k + 1], s[k:k + 1])), k


def test_ld4_launch_sequence(cuda, golden):
    """The fused test() of an L = 3 model issues, beside its convs, exactly L resized_mean_std
    and L ld4_fuse launches: no resize_nearest, no stand-alone AdaIN or statistics call, and
    no concatenation of feature maps."""
    g = golden("ld4")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    m.test(c, s)  # warm: the packed weights are cached
    names, cats = traced_launches(lambda: m.test(c, s))
    layers = int(g["net0_layers"])
    # conv launches are keyed '<algo><k>x<k> ...': everything else is listed here
    other = [nm for nm in names if not re.fullmatch(r"[a-z]+\d*x\d", nm.split(" ")[0])]
    assert len(other) < len(names)
    assert sorted(other) == sorted(
        [f"resized_mean_std C4 {h}x{w}->24x40 N4" for h, w in ((12, 20), (6, 10), (3, 5))] +
        [f"ld4_fuse {ca}+2x4 {h}x{w}->24x40 N2"
         for ca, (h, w) in ((0, (3, 5)), (8, (6, 10)), (8, (12, 20)))]), names
    assert len([nm for nm in names if nm.startswith("ld4_fuse")]) == layers
    assert not any(nm.startswith(("resize_nearest", "adain ", "stats ", "masked")) for nm in names)
    # the only concatenations: the AdaIN parameter vectors (1-D) and the two input images
    assert all(len(shape) == 1 or shape[1] == 3 for shapes in cats for shape in shapes), cats


def test_ld4_save_and_resume(cuda, golden, tmp_path):
    g = golden("ld4")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    y = m.test(c, s)
    path = str(tmp_path / "4321.pth")
    m.save(path, 4321)
    assert list(torch.load(path, weights_only=True).keys()) == list(m.state_dict().keys())
    import network as net
    cfg = dict(L4.config(4, 3, 0, 3), resume=True, checkpoint_path=path)
    m2 = net.LDMSAdaINRPNet4(cfg, copy.deepcopy(net.vgg)).to(cuda)
    assert m2.begin == 4321
    assert torch.equal(m2.test(c, s), y)


def test_ld4_forward_losses_under_no_grad(cuda, golden):
    g = golden("ld4")
    m = _net(g, 0, cuda)
    c, s = dev(g["net0_content"], cuda), dev(g["net0_style"], cuda)
    with torch.no_grad():
        losses, total = m(c, s)
    assert set(losses) == {"style_loss", "content_loss", "total_loss"}
    assert all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert torch.equal(total, losses["total_loss"])
    with pytest.raises(NotImplementedError, match="ld_adain4 training"):
        m(c, s)


# ---- pipeline -----------------------------------------------------------------------------
def test_pipeline_with_ld_adain4_and_masks(cuda, tmp_path):
    """stylize.py with `network: ld_adain4`, `use_mask: True`, `test_dataset: photoreal` and
    --synthetic-weights: the PNGs it writes are the direct test() call's through the pipeline's
    own uint8 conversion."""
    import network as net
    root = str(tmp_path / "data")
    # images 40 -> 32, masks 64 -> 32
    dataset_tree(root, 40, 64, ["L", "P"], rng_seed=14, mask_seed0=40)
    cfg = dict(L4.config(4, 3, 0, 1, True), network="ld_adain4", vgg="unused", img_size=32,
               test_dir=root, test_dataset="photoreal", batch_size=2, num_workers=2)
    m, _ = check_pipeline(cfg, tmp_path, cuda)
    assert isinstance(m, net.LDMSAdaINRPNet4)
