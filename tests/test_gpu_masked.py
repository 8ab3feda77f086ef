"""Segmentation-masked AdaIN on the GPU: the plan / params / apply kernels against the
float64 restatement (tests/masked_ref.py) and the reference goldens
(tests/golden/masked.*), the two networks' masked test() against the goldens, and the
pipeline with masks."""
import copy

import numpy as np
import pytest
import torch

import masked_ref as M
from helpers import (SOURCE_CONFIG, TOL_STATS, check_net, check_pipeline, dataset_tree, dev,
                     golden_net, mask_kw, multiscale_config, rel_l2, state_dict_of, synth_,
                     unfused)

pytestmark = pytest.mark.gpu


# ---- segment_plan ------------------------------------------------------------------------
def _map_of(counts, shape, seed):
    """A label map of `shape` holding exactly counts[label] pixels of each label, shuffled."""
    flat = np.concatenate([np.full(n, lab, np.uint8) for lab, n in counts.items()])
    assert flat.size == shape[0] * shape[1], (flat.size, shape)
    return np.random.default_rng(seed).permutation(flat).reshape(shape)


# label: (content count, style count) -> valid?
PLAN_CASE = {
    0: (20, 20, 1),       # label 0
    255: (30, 30, 1),     # label 255
    1: (10, 50, 0),       # 10 pixels: not more than 10
    2: (11, 11, 1),       # 11 pixels
    3: (1100, 11, 0),     # c / s exactly 100
    4: (1099, 11, 1),     # just under
    7: (11, 1100, 0),     # s / c exactly 100
    8: (11, 1099, 1),
    5: (50, 0, 0),        # content only
    6: (0, 50, 0),        # style only
}


@pytest.mark.parametrize("pad", [0, 1])  # HW a multiple of 4 (32-bit label loads) or not
def test_segment_plan_counts_and_flags(cuda, pad):
    from rpst import ops
    c_counts = {lab: v[0] for lab, v in PLAN_CASE.items() if v[0]}
    s_counts = {lab: v[1] for lab, v in PLAN_CASE.items() if v[1]}
    # filler label 9 brings the maps to (h, w); the style map has another size
    c_shape, s_shape = (34 + pad, 70), (50, 48 + pad)
    c_counts[9] = c_shape[0] * c_shape[1] - sum(c_counts.values())
    s_counts[9] = s_shape[0] * s_shape[1] - sum(s_counts.values())
    assert (c_shape[0] * c_shape[1]) % 4 == (2 * pad) % 4
    c0, s0 = _map_of(c_counts, c_shape, 1), _map_of(s_counts, s_shape, 2)
    # image 1: other masks (piecewise constant, labels 0 / 3 / 200 in rows)
    c1 = np.repeat(np.array([0, 3, 200, 3, 0], np.uint8), [5, 9, 10, 6, c_shape[0] - 30])
    c1 = np.tile(c1[:, None], (1, c_shape[1]))
    s1 = np.full(s_shape, 3, np.uint8)
    s1[:2, :5] = 200  # 10 pixels of 200 in the style: not valid
    plan = ops.segment_plan(dev(np.stack([c0, c1]), cuda), dev(np.stack([s0, s1]), cuda))
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (2, 256, 4)
    plan = plan.cpu().numpy()
    for n, (c, s) in enumerate([(c0, s0), (c1, s1)]):
        assert np.array_equal(plan[n, :, :3], M.label_counts(c, s)), n
    for lab, (cc, sc, valid) in PLAN_CASE.items():
        assert tuple(plan[0, lab, :3]) == (cc, sc, valid), lab
    assert plan[1, 3, 2] == 1 and plan[1, 200, 2] == 0 and plan[1, 0, 2] == 0
    assert plan[1, 0, 0] == (c_shape[0] - 25) * c_shape[1]


def test_masked_ops_reject_cpu_tensors():
    from rpst import ops
    seg = torch.zeros((1, 4, 4), dtype=torch.uint8)
    x = torch.zeros((1, 2, 4, 4))
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        ops.segment_plan(seg, seg)
    with pytest.raises(RuntimeError, match="ROCm GPU only"):
        ops.masked_adain(x, x, seg, seg)


# ---- masked_adain_params -----------------------------------------------------------------
def _op_cases(g):
    return [(i, str(g[f"op{i}_name"])) for i in range(int(g["n_ops"]))]


@pytest.fixture(scope="module")
def op_refs(golden):
    """Float64 restatement of every golden op case, computed once: case -> (rows (N, C, 256,
    4), counts (N, 256, 3))."""
    g = golden("masked")
    refs = {}
    for i, _ in _op_cases(g):
        per = [M.masked_params(g[f"op{i}_c"][n], g[f"op{i}_s"][n], g[f"op{i}_cseg"][n],
                               g[f"op{i}_sseg"][n]) for n in range(g[f"op{i}_c"].shape[0])]
        refs[i] = (np.stack([p[0] for p in per]), np.stack([p[1] for p in per]))
    return refs


def test_op_cases_cover_the_shapes(golden):
    g = golden("masked")
    shapes = {tuple(g[f"op{i}_c"].shape) for i, _ in _op_cases(g)}
    assert {(2, 8, 24, 40), (1, 3, 13, 9), (1, 40, 17, 33)} <= shapes
    assert any(g[f"op{i}_c"].shape[2:] != g[f"op{i}_s"].shape[2:] for i, _ in _op_cases(g))


def test_masked_adain_params_vs_float64(cuda, golden, op_refs):
    from rpst import ops
    g = golden("masked")
    for i, name in _op_cases(g):
        c, s = dev(g[f"op{i}_c"], cuda), dev(g[f"op{i}_s"], cuda)
        cseg, sseg = dev(g[f"op{i}_cseg"], cuda), dev(g[f"op{i}_sseg"], cuda)
        got = ops.masked_adain_params(c, s, cseg, sseg).cpu().numpy()
        rows, counts = op_refs[i]
        assert got.shape == rows.shape
        valid = counts[:, None, :, 2].astype(bool) & np.ones(rows.shape[:3], bool)
        assert valid.any()
        err = rel_l2(got[valid], rows[valid])
        print(f"params {name}: rel-L2 {err:.3e} over {int(valid.sum())} rows")
        assert err < TOL_STATS, (name, err)
        # every row of a label that is not valid is the pass-through row, exactly
        assert np.array_equal(got[~valid], rows[~valid]), name
        if name.startswith("sizes"):
            assert c.shape[2:] != s.shape[2:]


def test_single_label_agrees_with_calc_mean_std(cuda, golden):
    """One label over the whole map: the per-label statistics are the plane's, and sit within
    1 ulp of calc_mean_std's (the guarantee rpst_stats.hip states)."""
    from rpst import ops
    g = golden("masked")
    i = [k for k, name in _op_cases(g) if name.startswith("single")][0]
    c, s = dev(g[f"op{i}_c"], cuda), dev(g[f"op{i}_s"], cuda)
    lab = int(g[f"op{i}_cseg"][0, 0, 0])
    assert (g[f"op{i}_cseg"] == lab).all() and (g[f"op{i}_sseg"] == lab).all()
    p = ops.masked_adain_params(c, s, dev(g[f"op{i}_cseg"], cuda),
                                dev(g[f"op{i}_sseg"], cuda))[:, :, lab].cpu().numpy()
    cm, cs = (t.cpu().numpy().reshape(p.shape[:2]) for t in ops.calc_mean_std(c))
    sm, ss = (t.cpu().numpy().reshape(p.shape[:2]) for t in ops.calc_mean_std(s))
    for got, ref in ((p[..., 0], cm), (p[..., 1], cs), (p[..., 2], ss), (p[..., 3], sm)):
        assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()


# ---- masked_adain ------------------------------------------------------------------------
def test_masked_adain_vs_reference_goldens(cuda, golden, op_refs):
    from rpst import ops
    g = golden("masked")
    for i, name in _op_cases(g):
        c, s = dev(g[f"op{i}_c"], cuda), dev(g[f"op{i}_s"], cuda)
        cseg, sseg = dev(g[f"op{i}_cseg"], cuda), dev(g[f"op{i}_sseg"], cuda)
        out = ops.masked_adain(c, s, cseg, sseg)
        err = rel_l2(out, g[f"op{i}_out"])
        print(f"masked_adain {name}: rel-L2 {err:.3e}")
        assert err < TOL_STATS, (name, err)
        # pixels of labels that are not valid are the content's, bit for bit
        counts = op_refs[i][1]
        keep = np.stack([~counts[n][:, 2].astype(bool)[g[f"op{i}_cseg"][n]]
                         for n in range(c.shape[0])])
        keep = torch.from_numpy(keep).to(cuda)[:, None].expand_as(c)
        if not name.startswith(("stripes", "single")):
            assert keep.any() and not keep.all()
        assert torch.equal(out[keep], c[keep]), name
        assert not torch.equal(out[~keep], c[~keep]), name
        # two runs give the same bits
        assert torch.equal(out, ops.masked_adain(c, s, cseg, sseg)), name
        # with a skip tensor: skip + (the result without), rounded once in fp32
        skip = torch.from_numpy(np.random.default_rng(i).standard_normal(
            tuple(c.shape)).astype(np.float32)).to(cuda)
        plan = ops.segment_plan(cseg, sseg)
        with_skip = ops.masked_adain(c, s, cseg, sseg, skip=skip, plan=plan)
        assert torch.equal(with_skip, skip + out), name
        # out= is honoured
        buf = torch.empty_like(c)
        assert ops.masked_adain(c, s, cseg, sseg, plan=plan, out=buf) is buf
        assert torch.equal(buf, out)


def test_masked_adain_batch_independent(cuda, golden):
    from rpst import ops
    g = golden("masked")
    c, s = dev(g["op0_c"], cuda), dev(g["op0_s"], cuda)
    cseg, sseg = dev(g["op0_cseg"], cuda), dev(g["op0_sseg"], cuda)
    assert c.shape[0] == 2
    both = ops.masked_adain(c, s, cseg, sseg)
    for n in range(2):
        one = ops.masked_adain(c[n:n + 1], s[n:n + 1], cseg[n:n + 1], sseg[n:n + 1])
        assert torch.equal(both[n:n + 1], one), n


# ---- networks ----------------------------------------------------------------------------
MASK_FILE = "{tag}_{mode}_{b}.png"


@pytest.mark.parametrize("mode", ["L", "P"])
def test_multiscale_masked_golden(cuda, golden, tmp_path, mode):
    import network as net
    import network.adain_rp as arp
    g = golden("masked")
    m = golden_net(net.MultiScaleAdaINRPNet, dict(multiscale_config(8, 5, 0), use_mask=True), g,
                   "ms_", cuda)
    c, s = dev(g["ms_content"], cuda), dev(g["ms_style"], cuda)
    kw = mask_kw(g, "ms_", cuda, tmp_path, mode, MASK_FILE)
    y = m.test(c, s, **kw)
    check_net(y, g[f"ms_out_{mode}"], f"multiscale fused {mode}")
    # already-decoded label maps: the same bits as the paths
    cseg, sseg = dev(g[f"ms_cseg_{mode}"], cuda), dev(g[f"ms_sseg_{mode}"], cuda)
    assert torch.equal(m.test(c, s, c_mask_path=cseg, s_mask_path=sseg), y)
    assert torch.equal(m.test(c, s, c_mask_path=cseg.cpu(), s_mask_path=sseg.cpu()), y)
    # op by op: test() with FUSED_ADAIN off goes through decode(..., use_mask=True)
    with unfused(arp, "FUSED_ADAIN"):
        plain = m.test(c, s, **kw)
    check_net(plain, g[f"ms_out_{mode}"], f"multiscale op-by-op {mode}")
    with torch.no_grad():
        cf, sf = m.encode_rp_intermediate(c), m.encode_rp_intermediate(s)
        dec = m.decode(cf, sf, use_mask=True, **kw)
    assert torch.equal(dec, plain)


def test_multiscale_unmasked_unchanged_and_sort_still_raises(cuda, golden):
    """use_mask False ignores the mask arguments; shuffle / sort keep raising."""
    import network as net
    g = golden("masked")
    m = net.MultiScaleAdaINRPNet(multiscale_config(8, 5, 0), copy.deepcopy(net.vgg))
    synth_(m, int(g["ms_seed"]))
    m = m.to(cuda)
    c, s = dev(g["ms_content"], cuda), dev(g["ms_style"], cuda)
    cseg = dev(g["ms_cseg_P"], cuda)
    assert torch.equal(m.test(c, s), m.test(c, s, c_mask_path=cseg, s_mask_path=cseg))
    cfg = dict(multiscale_config(8, 5, 0), use_mask=True, sort=True)
    m2 = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg)).to(cuda)
    with pytest.raises(NotImplementedError):
        m2.test(c, s, c_mask_path=cseg, s_mask_path=cseg)


@pytest.mark.parametrize("mode", ["L", "P"])
def test_sourcenet_masked_golden(cuda, golden, tmp_path, mode):
    import network as net
    import network.base as base
    g = golden("masked")
    m = golden_net(net.SourceNet, dict(SOURCE_CONFIG, use_mask=True), g, "src_", cuda)
    c, s = dev(g["src_content"], cuda), dev(g["src_style"], cuda)
    kw = mask_kw(g, "src_", cuda, tmp_path, mode, MASK_FILE)
    y = m.test(c, s, **kw)
    check_net(y, g[f"src_out_{mode}"], f"sourcenet fused {mode}")
    cseg, sseg = dev(g[f"src_cseg_{mode}"], cuda), dev(g[f"src_sseg_{mode}"], cuda)
    assert tuple(cseg.shape) == (1, 8, 6)
    assert torch.equal(m.test(c, s, c_mask_path=cseg, s_mask_path=sseg), y)
    with unfused(base, "FUSED"):
        plain = m.test(c, s, **kw)
    check_net(plain, g[f"src_out_{mode}"], f"sourcenet op-by-op {mode}")


# ---- pipeline ----------------------------------------------------------------------------
def test_pipeline_with_masks_matches_direct_test(cuda, tmp_path):
    from rpst.imageio import to_uint8
    root = str(tmp_path / "data")
    # images 40 -> 32, masks 64 -> 32
    dataset_tree(root, 40, 64, ["L", "P"], rng_seed=11, mask_seed0=20)
    cfg = dict(multiscale_config(8, 3, 0), network="multi_adain", vgg="unused", use_mask=True,
               img_size=32, test_dir=root, test_dataset="photoreal", batch_size=2,
               num_workers=2)
    m, items = check_pipeline(cfg, tmp_path, cuda)
    # the masks matter: the unmasked network writes other pixels
    m.config["use_mask"] = False
    for c, s, ref in items:
        assert not np.array_equal(to_uint8(m.test(c, s))[0].cpu().numpy(), ref)


# ---- past one loop stride and one apply chunk ---------------------------------------------
# The shapes above keep every per-plane loop of rpst_masked.hip at one iteration. These are the
# smallest at which they repeat (masked_ref.STRIDE_SHAPES); masked_ref.run_path_census, a
# mirror of the statistics kernel's slicing, says which of its paths each label map reaches,
# and the conditions asserted on it are conditions on the inputs.
STRIDE_CASES = list(M.STRIDE_SHAPES)


def test_stride_cases_reach_every_path():
    cen = {name: M.stride_case(name).census for name in STRIDE_CASES}
    for name, c in cen.items():
        print(f"census {name}: {c}  style: {M.stride_case(name).style_census}")
    for kind in ("register", "element_later", "reg_to_elem", "elem_to_reg", "mixed_words",
                 "partial_waves"):
        assert any(cen[n][kind] > 0 for n in STRIDE_CASES if n != "e"), kind
    a = cen["a-bands"]
    assert a["register"] >= 10 and a["reg_to_elem"] >= 1 and a["elem_to_reg"] >= 1
    assert a["max_steps"] == 3 and a["apply_chunks"] == 3 and a["histogram_steps"] == 10
    assert cen["a-speckle"]["register"] == 0
    assert cen["a-speckle"]["mixed_words"] == 256 * 160 // 4  # every word
    assert cen["a-mixed"]["mixed_words"] > 0
    mixed = M.stride_case("a-mixed")
    assert tuple(mixed.counts[0, M.MIXED_STAMP]) == (10, 10, 0)
    assert mixed.counts[0, 0, 2] == 1 and mixed.counts[0, 255, 2] == 1
    assert cen["b"]["max_steps"] == 3 and cen["b"]["partial_waves"] == 0
    assert cen["b"]["reg_to_elem"] >= 1
    assert cen["c"]["partial_waves"] > 0 and cen["c"]["max_steps"] == 2
    assert cen["c"]["apply_chunks"] == 2
    c = M.stride_case("c")
    assert not np.array_equal(c.c_segs[0], c.c_segs[1])
    assert not np.array_equal(c.s_segs[0], c.s_segs[1])
    d = M.stride_case("d")
    assert d.style.shape[2:] != d.content.shape[2:]
    assert d.style_census["max_steps"] != cen["d"]["max_steps"]
    e = cen["e"]
    assert e["max_steps"] >= 2 and e["register"] == 0 and e["apply_chunks"] == 2
    assert (131 * 133) % 4


def _chunks(a, size):
    """(N, C, h, w) -> the planes flattened and cut at multiples of `size`."""
    flat = torch.as_tensor(a).reshape(a.shape[0], a.shape[1], -1)
    return [flat[..., o:o + size] for o in range(0, flat.shape[-1], size)]


@pytest.mark.parametrize("name", STRIDE_CASES)
def test_masked_kernels_past_one_stride(cuda, name):
    from rpst import ops
    case = M.stride_case(name)
    c, s, skip = case.content.to(cuda), case.style.to(cuda), case.skip.to(cuda)
    cseg, sseg = dev(case.c_segs, cuda), dev(case.s_segs, cuda)
    N = c.shape[0]
    # plan: counts and validity flags, exactly
    plan = ops.segment_plan(cseg, sseg)
    assert np.array_equal(plan.cpu().numpy()[:, :, :3], case.counts), name
    # parameters: pooled, then row by row (a pooled norm over hundreds of rows hides one label)
    got = ops.masked_adain_params(c, s, cseg, sseg).cpu().numpy()
    valid = case.counts[:, None, :, 2].astype(bool) & np.ones(case.rows.shape[:3], bool)
    err = rel_l2(got[valid], case.rows[valid])
    em, es = (max(v) for v in zip(*(M.row_errors(got[n], case.rows[n], case.counts[n])
                                    for n in range(N))))
    print(f"params {name}: rel-L2 {err:.3e} over {int(valid.sum())} rows, worst row mean "
          f"{em:.3e} std {es:.3e}")
    assert err < TOL_STATS, (name, err)
    assert em <= TOL_STATS and es <= TOL_STATS, (name, em, es)
    assert valid.any() and np.array_equal(got[~valid], case.rows[~valid]), name
    # output: pooled, then every apply chunk of 16384 elements by itself
    out = ops.masked_adain(c, s, cseg, sseg)
    err = rel_l2(out, case.out)
    per = [rel_l2(g, r) for g, r in zip(_chunks(out.cpu(), M.APPLY_ELEMS),
                                        _chunks(case.out, M.APPLY_ELEMS))]
    print(f"masked_adain {name}: rel-L2 {err:.3e}, per chunk "
          + " ".join(f"{e:.3e}" for e in per))
    assert err < TOL_STATS, (name, err)
    assert len(per) == case.census["apply_chunks"] and max(per) < TOL_STATS, (name, per)
    keep = np.stack([~case.counts[n][:, 2].astype(bool)[case.c_segs[n]] for n in range(N)])
    keep = torch.from_numpy(keep).to(cuda)[:, None].expand_as(c)
    assert torch.equal(out[keep], c[keep]), name
    if name == "a-mixed":
        assert int(keep[0, 0].sum()) == 10
    assert not torch.equal(out[~keep], c[~keep]), name
    assert torch.equal(out, ops.masked_adain(c, s, cseg, sseg)), name
    assert torch.equal(ops.masked_adain(c, s, cseg, sseg, skip=skip, plan=plan), skip + out)
    buf = torch.empty_like(c)
    assert ops.masked_adain(c, s, cseg, sseg, plan=plan, out=buf) is buf
    assert torch.equal(buf, out)
    if N > 1:  # each image alone is its slice of the batch, bit for bit
        for n in range(N):
            one = ops.masked_adain(c[n:n + 1], s[n:n + 1], cseg[n:n + 1], sseg[n:n + 1])
            assert torch.equal(out[n:n + 1], one), (name, n)


def test_single_label_agrees_with_calc_mean_std_with_carried_runs(cuda):
    """test_single_label_agrees_with_calc_mean_std where the runs are carried in registers
    across steps: one label over (256, 160), 3 steps a slice, all but the first on the
    register path."""
    from rpst import ops
    shape, lab = (1, 2, 256, 160), 60
    seg = np.full((1, 256, 160), lab, np.uint8)
    cen = M.run_path_census(seg[0], shape[1])
    # 16 slices x (4 waves in the second step + the 2 active ones in the third)
    assert cen["register"] == 96 and cen["element_later"] == 0 and cen["max_steps"] == 3
    c = M.labelled_feature(171, shape, seg).to(cuda)
    s = (M.labelled_feature(172, shape, seg) * 0.7 + 0.5).to(cuda)
    p = ops.masked_adain_params(c, s, dev(seg, cuda), dev(seg, cuda))[:, :, lab].cpu().numpy()
    cm, cs = (t.cpu().numpy().reshape(p.shape[:2]) for t in ops.calc_mean_std(c))
    sm, ss = (t.cpu().numpy().reshape(p.shape[:2]) for t in ops.calc_mean_std(s))
    for got, ref in ((p[..., 0], cm), (p[..., 1], cs), (p[..., 2], ss), (p[..., 3], sm)):
        assert (np.abs(got - ref) <= np.spacing(np.abs(ref))).all()


def test_multiscale_masked_at_136x128_vs_float64(cuda):
    """One plan over every level of MultiScaleAdaINRPNet.test at a size where each level's
    kernels repeat (case c's maps: 2 statistics steps with a partly active wave, 2 apply
    chunks), against the float64 restatement on the same state dict."""
    import network as net
    case = M.stride_case("c")
    m = net.MultiScaleAdaINRPNet(dict(multiscale_config(8, 5, 0), use_mask=True),
                                 copy.deepcopy(net.vgg))
    synth_(m, 33)
    sd = {k: v.double() for k, v in state_dict_of(m).items()}
    from helpers import gen
    c, s = gen(181, (2, 3, 136, 128), 0.5, 0.5), gen(182, (2, 3, 136, 128), 0.5, 0.5)
    ref = M.multiscale_test(c.double(), s.double(), sd, 5, case.c_segs, case.s_segs)
    assert ref.dtype == torch.float64
    m = m.to(cuda)
    y = m.test(c.to(cuda), s.to(cuda), c_mask_path=dev(case.c_segs, cuda),
               s_mask_path=dev(case.s_segs, cuda))
    check_net(y, ref, "multiscale masked 136x128 vs float64")
