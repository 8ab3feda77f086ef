"""LDMSAdaINRPNet4 (`network: ld_adain4`), the parts that need no GPU: the float64 restatement
(tests/ld4_ref.py) against the reference's recorded float64 outputs and levels, the mirror's
state_dict keys, the host statement of the nearest rule against torch's CPU kernel, the
argument checks of the three ABI entries, and what keeps raising."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ld4_ref as L4
import ld_ref as L
from helpers import TOL_STATS, gen, golden_net, rel_l2


def _model(g, i):
    import network as net
    return golden_net(net.LDMSAdaINRPNet4, L4.golden_config(g, i), g, f"net{i}_")


def test_cases_recorded(golden):
    g = golden("ld4")
    assert int(g["n_net"]) == len(L4.CASES) == 6
    for i, (hid, layers, inc, shape, sl, use_mask, seed) in enumerate(L4.CASES):
        assert (int(g[f"net{i}_hidden"]), int(g[f"net{i}_layers"]), int(g[f"net{i}_inception"]),
                tuple(g[f"net{i}_content"].shape), int(g[f"net{i}_stylized_layers"]),
                bool(g[f"net{i}_use_mask"]), int(g[f"net{i}_seed"])) == (
                    hid, layers, inc, shape, sl, use_mask, seed)
        # the reference's own fp32 distance sits far inside TOL_NET and the level bar
        assert float(g[f"net{i}_floor"]) < 1e-5, i
        assert all(float(g[f"net{i}_level{k}_floor"]) < 3e-6 for k in range(layers)), i
        assert bool(g[f"net{i}_has_levels"]) == (
            L4.level_bytes(hid, layers, shape) < L4.LEVEL_BYTES)
    # the masked case is the unmasked one's model and images
    assert np.array_equal(g["net0_checksum"], g["net1_checksum"])
    assert np.array_equal(g["net0_content"], g["net1_content"])
    assert not np.array_equal(g["net0_out"], g["net1_out"])


@pytest.mark.parametrize("i", range(len(L4.CASES)))
def test_restatement_matches_reference_float64(golden, i):
    """ld4_ref.test / ld4_ref.encode against the reference's float64 run: 1e-9 rel-L2 for the
    output and for every recorded level of encode_rp_intermediate(content)."""
    g = golden("ld4")
    m = _model(g, i)  # (its checksum is the recorded one)
    sd = m.state_dict()
    layers, hid = int(g[f"net{i}_layers"]), int(g[f"net{i}_hidden"])
    segs = (g[f"net{i}_cseg"], g[f"net{i}_sseg"]) if bool(g[f"net{i}_use_mask"]) else (None, None)
    y = L4.test(g[f"net{i}_content"], g[f"net{i}_style"], sd, layers, *segs)
    assert g[f"net{i}_out64"].dtype == np.float64
    err = rel_l2(y, g[f"net{i}_out64"])
    print(f"case {i}: restatement vs float64 reference {err:.2e}")
    assert err < 1e-9, (i, err)
    if bool(g[f"net{i}_has_levels"]):
        with torch.no_grad():
            levels = L4.encode(g[f"net{i}_content"], sd, layers)
        for k, lv in enumerate(levels):
            assert lv.shape[1] == 2 * hid
            assert rel_l2(lv, g[f"net{i}_level{k}_64"]) < 1e-9, (i, k)


@pytest.mark.parametrize("i", range(len(L4.CASES)))
def test_state_dict_keys_match_reference(golden, i):
    g = golden("ld4")
    m = _model(g, i)
    names, shapes = L4.key_table(m.state_dict())
    assert list(names) == list(g[f"net{i}_keys"])
    assert np.array_equal(shapes, g[f"net{i}_shapes"])
    big = [k for k in names if "_big_revf." in k]
    assert {k.split("_big_revf.")[1].split(".")[0] for k in big} == {"0", "2", "5"}


def test_modules_and_decoder_widths():
    import network as net
    h = 4
    for layers, sl, widths in ((3, 3, [(2 * h, 2 * h), (4 * h, 2 * h), (4 * h, 3)]),
                               (3, 1, [(2 * h, h), (3 * h, h), (3 * h, 3)]),
                               (4, 2, [(2 * h, 2 * h), (4 * h, h), (3 * h, h), (3 * h, 3)]),
                               (1, 1, [(2 * h, 3)])):
        m = net.LDMSAdaINRPNet4(L4.config(h, layers, 0, sl), copy.deepcopy(net.vgg))
        got = [(getattr(m, f"rp_dec{k}").conv.in_channels,
                getattr(m, f"rp_dec{k}").conv.out_channels) for k in range(layers)]
        assert got == widths, (layers, sl, got)
        assert isinstance(m.rp_enc0_big_revf, torch.nn.Sequential)
        assert isinstance(m.rp_enc0_small_revf, net.Conv2dBlock)
        assert m.rp_shared_encoder is None and m.rp_decoder is None
        assert isinstance(m, net.LDMSAdaINRPNet)


def test_stylized_layers_out_of_range_raises():
    import network as net
    for sl in (0, 4):
        with pytest.raises(ValueError, match="stylized_layers"):
            net.LDMSAdaINRPNet4(L4.config(4, 3, 0, sl), copy.deepcopy(net.vgg))
    # LDMSAdaINRPNet keeps its own rule
    with pytest.raises(ValueError, match="stylized_layers"):
        net.LDMSAdaINRPNet(L4.config(4, 3, 0, 2), copy.deepcopy(net.vgg))


# ---- the nearest rule -----------------------------------------------------------------------
def _torch_index(size_in, size_out):
    src = torch.arange(size_in, dtype=torch.float32).view(1, 1, 1, size_in)
    return F.interpolate(src, (1, size_out))[0, 0, 0].to(torch.int32)


def _pairs():
    pairs = [(i, o) for o in range(1, 131) for i in range(1, o + 1)]
    for s in (512, 1000, 1024):
        pairs += [(-(-s // 2 ** k), s) for k in range(1, 6)] + [(s, s)]
    return pairs


def test_index_table_equals_torch_interpolate():
    """ops.nearest_index_table (the kernels' statement of the rule, run on the host) against
    F.interpolate of an arange: every 1 <= in <= out <= 130, the pyramid sizes of 512 / 1000 /
    1024, and out = in; the restatement's numpy form as well; the counts sum to `out`."""
    from rpst import ops
    for size_in, size_out in _pairs():
        want = _torch_index(size_in, size_out)
        got = ops.nearest_index_table(size_in, size_out)
        assert got.dtype == torch.int32 and torch.equal(got, want), (size_in, size_out)
        assert np.array_equal(L4.nearest_index(size_in, size_out), want.numpy()), (size_in, size_out)
        if size_in == size_out:
            assert torch.equal(got, torch.arange(size_in, dtype=torch.int32))


def test_replication_counts_sum_to_out():
    from rpst import ops
    for size_in, size_out in _pairs()[::7] + [(1, 1), (3, 130), (17, 1000)]:
        counts = ops.nearest_counts(size_in, size_out)
        assert tuple(counts.shape) == (size_in,) and int(counts.sum()) == size_out
        assert torch.equal(counts, torch.bincount(_torch_index(size_in, size_out).long(),
                                                  minlength=size_in))


def test_two_dimensional_resize_is_separable():
    """F.interpolate(x, (H, W)) is the row table applied to rows and the column table to columns
    (what the kernels and ld4_ref.resize_nearest assume)."""
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    for size in ((5, 7), (19, 37), (10, 14), (6, 50)):
        assert torch.equal(L4.resize_nearest(x, size), F.interpolate(x, size))
        assert torch.equal(L4.resize_nearest(x.double(), size), F.interpolate(x.double(), size))


# ---- what raises ----------------------------------------------------------------------------
def test_stylize_builds_ld_adain4_and_refuses_the_others():
    import network as net
    import stylize
    import train
    opt = dict(L4.config(4, 3, 0, 1, True), network="ld_adain4")
    assert isinstance(stylize.build_network(opt, synthetic_seed=1), net.LDMSAdaINRPNet4)
    assert "ld_adain4" not in stylize.OUT_OF_SCOPE and "ld_adain4" in stylize.MASKED_NETWORKS
    assert stylize.mask_size("ld_adain4", 24) == (24, 24)
    for kind in ("ld_adain2", "ld_adain3", "ld_adain5", "sel_multi_adain", "mrf", "spade"):
        with pytest.raises(NotImplementedError):
            stylize.build_network(dict(opt, network=kind), synthetic_seed=1)
    assert "ld_adain4" not in train.TRAINABLE


def test_ops_refuse_cpu_tensors():
    from rpst import ops
    src = torch.zeros(1, 4, 3, 4)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.resize_nearest(src, (5, 7))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.resized_mean_std(src, (5, 7))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        ops.ld4_fuse(None, torch.zeros(1, 4, 5, 7), src, torch.zeros(16), torch.zeros(16))


def test_forward_with_grad_raises():
    import network as net
    m = net.LDMSAdaINRPNet4(L4.config(4, 3), copy.deepcopy(net.vgg))
    x = torch.zeros(1, 3, 8, 8)
    assert torch.is_grad_enabled() and any(p.requires_grad for p in m.parameters())
    with pytest.raises(NotImplementedError, match="ld_adain4 training"):
        m(x, x)
    with torch.no_grad():  # op by op: the kernels refuse the CPU tensors, nothing falls back
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            m(x, x)
    for key in ("sort", "shuffle"):
        cfg = L4.config(4, 3)
        cfg[key] = True
        with pytest.raises(NotImplementedError, match="shuffle / sort"):
            net.LDMSAdaINRPNet4(cfg, copy.deepcopy(net.vgg))(x, x)


def test_abi_argument_errors():
    """The three entries check their arguments before touching the device."""
    from rpst import _lib
    lib = _lib.load()

    def err():
        return lib.rpst_last_error().decode()

    def resize(src=1, dst=1, N=1, C=4, h=3, w=4, H=5, W=7, off=0, total=4):
        return lib.rpst_resize_nearest(src, dst, N, C, h, w, H, W, off, total, None)

    assert resize(src=None) == -1 and "null pointer" in err()
    assert resize(dst=None) == -1 and "null pointer" in err()
    assert resize(N=0) == -1 and "bad shape" in err()
    assert resize(off=1) == -1 and "channels" in err()
    assert resize(off=4, total=7) == -1 and "channels" in err()
    assert resize(off=-1, total=8) == -1 and "channels" in err()
    assert resize(h=6) == -1 and "enlarges only" in err()
    assert resize(w=8) == -1 and "enlarges only" in err()

    def stats(src=1, mean=1, std=1, N=1, C=4, h=3, w=4, H=5, W=7, ws=1, nbytes=28):
        return lib.rpst_resized_mean_std(src, mean, std, N, C, h, w, H, W, 1e-5, ws, nbytes, None)

    assert lib.rpst_resized_mean_std_workspace_size(3, 4) == 28
    assert lib.rpst_resized_mean_std_workspace_size(0, 4) == 0
    assert stats(src=None) == -1 and "null pointer" in err()
    assert stats(std=None) == -1 and "null pointer" in err()
    assert stats(C=0) == -1 and "bad shape" in err()
    assert stats(h=6) == -1 and "enlarges only" in err()
    assert stats(nbytes=27) == -3 and "workspace" in err()
    assert stats(ws=None) == -3 and "workspace" in err()

    def fuse(y=None, fine=1, coarse=1, pf=1, pc=1, out=1, N=1, Ca=0, hid=4, H=5, W=7, h=3, w=4):
        return lib.rpst_ld4_fuse(y, fine, coarse, pf, pc, out, N, Ca, hid, H, W, h, w, None)

    assert fuse(fine=None) == -1 and "null pointer" in err()
    assert fuse(pc=None) == -1 and "null pointer" in err()
    assert fuse(out=None) == -1 and "null pointer" in err()
    assert fuse(Ca=4) == -1 and "y must be given" in err()
    assert fuse(y=1) == -1 and "y must be given" in err()
    assert fuse(Ca=-1) == -1 and "y must be given" in err()
    assert fuse(hid=0) == -1 and "bad shape" in err()
    assert fuse(h=6) == -1 and "enlarges only" in err()

    assert lib.rpst_nearest_index_table(3, 5, None) == -1 and "null pointer" in err()
    import ctypes
    buf = (ctypes.c_int * 4)()
    assert lib.rpst_nearest_index_table(0, 4, ctypes.addressof(buf)) == -1 and "bad sizes" in err()


# ---- the multi-chunk inputs tell a wrong walk from a right one -------------------------------
# float64 on the very inputs of tests/test_gpu_ld4.py's multi-chunk cases: each slip that those
# cases aim at, planted in ld4_ref's restatement of the kernels' walk, has to miss the bar it
# is meant to trip by a factor of TEETH (and to change bits, where the test asks for bit
# equality). The measured ratios: profiles/loop_strides/teeth.txt.
TEETH = 10.0
MULTI_RESIZE = [((2, 5, 33, 34), (65, 67)), ((1, 3, 23, 29), (65, 67)),
                ((1, 2, 40, 52), (91, 93)), ((1, 4, 64, 64), (128, 128))]
MULTI_FUSE = [((65, 67), (33, 34)), ((91, 93), (23, 29)), ((128, 128), (64, 64))]


def test_walk_restated_covers_every_element():
    """Without a slip write_planes is the identity, whatever the planes' heads; an odd plane
    size cycles the heads through 0, 3, 2, 1."""
    for hw, planes in ((4355, 10), (8463, 5), (16384, 3), (7, 4), (2, 3)):
        val = np.arange(1, planes * hw + 1, dtype=np.float64).reshape(planes, hw)
        for first in (0, 1):
            assert np.array_equal(L4.write_planes(val, first), val)
    assert [(-p * 4355) % 4 for p in range(4)] == [0, 1, 2, 3]
    assert L4.CHUNK == 4096 and 4355 > L4.CHUNK and 8463 > 2 * L4.CHUNK


def _plane_chunk_ratio(got, want):
    """The worst rel-L2 over (plane, chunk of 4096 elements) / TOL_STATS."""
    worst = 0.0
    for o in range(0, want.shape[1], L4.CHUNK):
        g, w = got[:, o:o + L4.CHUNK], want[:, o:o + L4.CHUNK]
        worst = max(worst, float((np.linalg.norm(g - w, axis=1) / np.linalg.norm(w, axis=1)).max()))
    return worst / TOL_STATS


def _slip_applies(slip, hw, planes):
    heads = {(-p * hw) % 4 for p in range(planes)}
    if slip == "no_head":
        return heads != {0}
    if slip == "no_tail":
        return any((hw - h) % 4 for h in heads)
    return hw > L4.CHUNK


@pytest.mark.parametrize("slip", ["chunk_base", "no_head", "no_tail"])
@pytest.mark.parametrize("shape,size", MULTI_RESIZE)
def test_teeth_resize_walk(shape, size, slip):
    """resize_nearest, alone and into the upper channel slice of a tensor twice as wide: the
    planted walk changes bits (the test asks for equality with F.interpolate)."""
    n, c = shape[:2]
    hw = size[0] * size[1]
    want = F.interpolate(gen(41, shape, 2.0, 0.5), size).double().numpy()
    for first, planes in ((0, want.reshape(-1, hw)), (c, want[0].reshape(-1, hw))):
        if not _slip_applies(slip, hw, first + len(planes)):
            assert slip != "chunk_base" and hw % 4 == 0  # aligned planes have no ragged ends
            continue
        got = L4.write_planes(planes, first, slip)
        assert not np.array_equal(got, planes)
        ratio = rel_l2(got, planes) / TOL_STATS
        print(f"teeth resize {shape}->{size} {slip} (first plane {first}): bits differ, "
              f"rel-L2 {ratio:.0f}x TOL_STATS")
        assert ratio >= TEETH


@pytest.mark.parametrize("slip", ["chunk_base", "no_head", "no_tail"])
@pytest.mark.parametrize("ca,hd", [(0, 4), (4, 5), (3, 5), (3, 4)])
@pytest.mark.parametrize("size,csize", MULTI_FUSE)
def test_teeth_fuse_walk(size, csize, ca, hd, slip):
    """ld4_fuse's output planes (y's, the fine half's, the gathered half's) written by the
    planted walk: the per-chunk bar of test_ld4_fuse_vs_float64 is missed."""
    n, hw = 2, size[0] * size[1]
    y, fine, coarse, stats = L4.fuse_inputs(ca, hd, size, csize, n)
    want = L4.fuse_want(fine, coarse, stats, size, n)
    full = want if y is None else torch.cat([y.double(), want], dim=1)
    planes = full.numpy().reshape(-1, hw)
    if not _slip_applies(slip, hw, len(planes)):
        assert slip != "chunk_base" and hw % 4 == 0
        return
    got = L4.write_planes(planes, 0, slip).reshape(n, ca + 2 * hd, hw)
    ratio = _plane_chunk_ratio(got[:, ca:].reshape(-1, hw), want.numpy().reshape(-1, hw))
    print(f"teeth fuse {ca}+2x{hd} {csize}->{size} {slip}: chunk bar missed by {ratio:.0f}x")
    assert ratio >= TEETH


@pytest.mark.parametrize("shape,size", MULTI_RESIZE)
def test_teeth_resized_statistics(shape, size):
    """resized_mean_std: the restated weighted sums are the statistics of the resized map
    (1e-11), and stopping after one stride of 256 quads, or skipping the 0-3 tail elements,
    misses TOL_STATS."""
    x = gen(42, shape, 2.0, 0.5)
    rm, rs = L.mean_std(F.interpolate(x, size).double())
    m, s = L4.resized_stats(x, size)
    assert rel_l2(m, rm) < 1e-11 and rel_l2(s, rs) < 1e-11
    hw = shape[2] * shape[3]
    # ((23, 29) is there for its ratios: 166 quads, one stride, and a 3-element tail)
    assert hw // 4 > L4.STRIDE_QUADS or shape == (1, 3, 23, 29)
    slips = (["one_stride"] if hw // 4 > L4.STRIDE_QUADS else []) + (["no_tail"] if hw % 4 else [])
    for slip in slips:
        m, s = L4.resized_stats(x, size, slip)
        ratio = max(rel_l2(m, rm), rel_l2(s, rs)) / TOL_STATS
        print(f"teeth resized_mean_std {shape}->{size} {slip}: TOL_STATS missed by {ratio:.0f}x")
        assert ratio >= TEETH
    if shape == (2, 5, 33, 34):
        assert slips == ["one_stride", "no_tail"] and hw % 4 == 2
