"""Segmentation-masked AdaIN without a GPU: the float64 restatement (tests/masked_ref.py)
against the reference goldens (tests/golden/masked.*, gen_golden_masked.py), and the mask
loader against the label arrays the reference saw."""
import copy

import numpy as np
import pytest
import torch

import masked_ref as M
from helpers import SOURCE_CONFIG, multiscale_config, rel_l2, state_dict_of, synth_

# The restatement against the reference's fp32 outputs. The masked op is restated in float64
# (the reference's own fp32-vs-float64 distance for it measures 7.8e-8); the networks' conv
# layers run through the oracle's restatement in fp32, as the reference runs them.
TOL_RESTATE = 1e-6


@pytest.fixture
def generator_threads():
    """The goldens' thread count (gen_golden_masked.py sets 8): torch's fp32 CPU convs round
    differently under another partition of the work, by about the bar itself through VGG."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def test_restatement_reproduces_op_goldens(golden):
    g = golden("masked")
    for i in range(int(g["n_ops"])):
        ref = M.masked_adain_batch(g[f"op{i}_c"], g[f"op{i}_s"], g[f"op{i}_cseg"],
                                   g[f"op{i}_sseg"])
        err = rel_l2(ref, g[f"op{i}_out"])
        print(f"op {i} {g[f'op{i}_name']}: rel-L2 {err:.3e}")
        assert err <= TOL_RESTATE, (i, err)
        # the case does something: some pixels move, and (but for the stripes and the single
        # label) some stay
        moved = np.any(g[f"op{i}_out"] != g[f"op{i}_c"], axis=1)
        assert moved.any()
        if str(g[f"op{i}_name"]).startswith(("blocks", "wide", "sizes", "odd")):
            assert not moved.all()


def test_restatement_reproduces_multiscale_goldens(golden, generator_threads):
    import network as net
    g = golden("masked")
    m = net.MultiScaleAdaINRPNet(dict(multiscale_config(8, 5, 0), use_mask=True),
                                 copy.deepcopy(net.vgg))
    assert np.array_equal(synth_(m, int(g["ms_seed"])), g["ms_checksum"])
    sd = state_dict_of(m)
    c, s = torch.from_numpy(g["ms_content"]), torch.from_numpy(g["ms_style"])
    for mode in ("L", "P"):
        y = M.multiscale_test(c, s, sd, 5, g[f"ms_cseg_{mode}"], g[f"ms_sseg_{mode}"])
        err = rel_l2(y, g[f"ms_out_{mode}"])
        print(f"multiscale {mode}: rel-L2 {err:.3e}")
        assert err <= TOL_RESTATE, (mode, err)
    assert not np.array_equal(g["ms_out_L"], g["ms_out_P"])


def test_restatement_reproduces_sourcenet_goldens(golden, generator_threads):
    """Measured: 7.9e-7 (L) / 8.4e-7 (P) on the CPU model the goldens were generated on, at any
    OMP thread count; 1.30e-6 (L) on an EPYC 9575F host, whose fp32 convs round differently:
    there the oracle's own unmasked checks at this bar (tests/test_oracle_golden.py:
    test_sourcenet_test 1.1e-6, test_vgg_and_decoder 1.3e-6) miss it in the same way. The
    masked op itself is restated to 6-8e-8 (test_restatement_reproduces_op_goldens)."""
    import network as net
    g = golden("masked")
    m = net.SourceNet(dict(SOURCE_CONFIG, use_mask=True), copy.deepcopy(net.vgg))
    assert np.array_equal(synth_(m, int(g["src_seed"])), g["src_checksum"])
    sd = state_dict_of(m)
    c, s = torch.from_numpy(g["src_content"]), torch.from_numpy(g["src_style"])
    for mode in ("L", "P"):
        assert g[f"src_cseg_{mode}"].shape == (1, 8, 6)
        y = M.sourcenet_test(c, s, sd, g[f"src_cseg_{mode}"], g[f"src_sseg_{mode}"])
        err = rel_l2(y, g[f"src_out_{mode}"])
        print(f"sourcenet {mode}: rel-L2 {err:.3e}")
        assert err <= TOL_RESTATE, (mode, err)


def _mask_sets(g):
    """(tag, mode, file-resolution maps, resized maps) of every golden mask."""
    for i in range(int(g["n_ops"])):
        for side in ("c", "s"):
            yield (f"op{i}{side}", str(g[f"op{i}_mode"]), g[f"op{i}_{side}file"],
                   g[f"op{i}_{side}seg"])
    for net in ("ms", "src"):
        for mode in ("L", "P"):
            for side in ("c", "s"):
                yield (f"{net}{side}{mode}", mode, g[f"{net}_{side}file"],
                       g[f"{net}_{side}seg_{mode}"])


def test_load_segment_reproduces_recorded_labels(golden, tmp_path):
    """Greyscale masks are resampled bicubically (in-between labels along the borders),
    palette masks by nearest neighbour: whatever this machine's Pillow does must be what the
    reference's Pillow did when the goldens were recorded."""
    from rpst.imageio import load_segment, load_segments
    g = golden("masked")
    invented = 0
    for tag, mode, files, segs in _mask_sets(g):
        paths = []
        for b in range(files.shape[0]):
            paths.append(M.write_mask_png(str(tmp_path / f"{tag}{b}.png"), files[b], mode))
            h, w = segs[b].shape
            got = load_segment(paths[-1], (w, h))
            assert got.dtype == np.uint8 and got.shape == (h, w)
            assert np.array_equal(got, segs[b]), (tag, b)
            if mode == "L" and files[b].shape != segs[b].shape:
                invented += len(set(np.unique(got)) - set(np.unique(files[b])))
            if mode == "P":
                assert set(np.unique(got)) <= set(np.unique(files[b]))
        both = load_segments(paths, (segs.shape[2], segs.shape[1]))
        assert both.dtype == torch.uint8 and np.array_equal(both.numpy(), segs)
    assert invented > 0  # the bicubic path was exercised


def test_load_segment_rejects_rgb_mask(tmp_path):
    from PIL import Image
    from rpst.imageio import load_segment
    p = str(tmp_path / "rgb.png")
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8)).save(p)
    with pytest.raises(ValueError, match="2-D"):
        load_segment(p, (4, 4))


def test_restatement_validity_rule():
    def plan(c_counts, s_counts):
        c = np.concatenate([np.full(n, lab, np.uint8) for lab, n in c_counts.items()])
        s = np.concatenate([np.full(n, lab, np.uint8) for lab, n in s_counts.items()])
        return M.label_counts(c[None], s[None])
    p = plan({1: 10, 2: 11, 3: 1100, 4: 1099, 5: 50}, {1: 50, 2: 11, 3: 11, 4: 11, 6: 50})
    assert [int(p[k, 2]) for k in (1, 2, 3, 4, 5, 6)] == [0, 1, 0, 1, 0, 0]
