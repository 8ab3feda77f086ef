"""Segmentation-masked AdaIN without a GPU: the float64 restatement (tests/masked_ref.py)
against the reference goldens (tests/golden/masked.*, gen_golden_masked.py), and the mask
loader against the label arrays the reference saw."""
import copy

import numpy as np
import pytest
import torch

import masked_ref as M
from helpers import (SOURCE_CONFIG, TOL_STATS, multiscale_config, rel_l2, state_dict_of,
                     synth_)

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


# ---- run_path_census on maps whose counts are worked out by hand ---------------------------
def test_census_of_hand_made_maps():
    base = dict(register=0, element_later=0, reg_to_elem=0, elem_to_reg=0, mixed_words=0,
                partial_waves=0, apply_chunks=1, histogram_steps=1)
    assert [M.masked_splits(c) for c in (1, 2, 32, 33, 64, 100, 512, 513, 2048)] == [
        16, 16, 16, 16, 8, 6, 1, 1, 1]
    # C = 512: one slice. 768 words, three full steps; label 1 up to word 512, then label 2.
    # Step 0: no lane has a label, 4 element wave-steps (first steps are not 'later'). Step 1:
    # words 256-511, all label 1: 4 register wave-steps after element ones. Step 2: lane 0
    # reads word 512 (label 1), every other lane label 2: no wave stays in its runs, all four
    # hand over runs carried since step 0.
    seg = np.repeat(np.array([1, 2], np.uint8), [4 * 513, 4 * 255]).reshape(1, -1)
    assert M.run_path_census(seg, 512) == dict(base, register=4, element_later=4,
                                               reg_to_elem=4, elem_to_reg=4, max_steps=3)
    cen = M.run_path_census(seg, 512, detail=True)
    assert cen["transitions"] == [(0, 2, 0), (0, 2, 1), (0, 2, 2), (0, 2, 3)]
    # lane 1 is wave 0's first to change: it carried words 1 and 257
    assert list(M.carried_run_elements(seg, 512, 0, 2, 0)) == [4, 5, 6, 7, 1028, 1029, 1030, 1031]
    # lane 64 (wave 1) carried words 64 and 320
    assert list(M.carried_run_elements(seg, 512, 0, 2, 1)) == [256, 257, 258, 259, 1280, 1281,
                                                               1282, 1283]
    # 528 words: steps of 256, 256 and 16 lanes. Label 1 on pixels 0-1025, so word 256 is
    # (1, 1, 2, 2). Step 1: lane 0 reads the mixed word, the others label 2 after label 1: 4
    # element wave-steps. Step 2: wave 0 alone, 16 of its lanes, all label 2 like their last
    # pixel: one register wave-step, partly active.
    seg = np.repeat(np.array([1, 2], np.uint8), [1026, 2112 - 1026]).reshape(3, 704)
    assert M.run_path_census(seg, 512) == dict(base, register=1, element_later=4,
                                               elem_to_reg=1, mixed_words=1, partial_waves=1,
                                               max_steps=3)
    # the same at C = 256: two slices of 264 words, each a full step and one of 8 lanes.
    # Slice 0 is label 1 throughout but for its last word, the mixed one, on lane 7 of step 1:
    # an element step after an element step. Slice 1 is label 2: a register step.
    assert M.run_path_census(seg, 256) == dict(base, register=1, element_later=1,
                                               elem_to_reg=1, mixed_words=1, partial_waves=2,
                                               max_steps=2)
    # 513 pixels, not a multiple of 4: pixel units, never the register path; steps of 256, 256
    # and 1 lanes
    seg = np.zeros((3, 171), np.uint8)
    assert M.run_path_census(seg, 512) == dict(base, element_later=5, partial_waves=1,
                                               max_steps=3)
    assert M.run_path_census(np.zeros((130, 128), np.uint8), 8)["apply_chunks"] == 2
    assert M.run_path_census(np.zeros((65, 64), np.uint8), 8)["histogram_steps"] == 2


# ---- the loop-stride inputs tell a wrong walk from a right one ------------------------------
# float64 numpy on the very inputs of tests/test_gpu_masked.py's stride cases: each slip that
# those tests aim at, planted in the restatement, has to miss the bar it is meant to trip by a
# factor of TEETH, so a kernel that passes at that bar does not have the slip. The measured
# ratios: profiles/loop_strides/teeth.txt.
TEETH = 10.0


def _row_ratio(case, n, drop):
    """max(row mean figure, row std figure) / TOL_STATS of image n's parameters with the
    content pixels `drop` left out of the sums."""
    got, _ = M.kernel_form_params(case.content[n].numpy(), case.style[n].numpy(),
                                  case.c_segs[n], case.s_segs[n], c_drop=drop)
    return max(M.row_errors(got, case.rows[n], case.counts[n])) / TOL_STATS


@pytest.mark.parametrize("name", list(M.STRIDE_SHAPES))
def test_kernel_form_is_the_restatement(name):
    """float64 rounding alone: the shifted sums cancel (d d up to 33^2 against a variance of
    0.05 and up), 1e-9 leaves four digits over that."""
    case = M.stride_case(name)
    for n in range(case.content.shape[0]):
        e = _row_ratio(case, n, None) * TOL_STATS
        print(f"kernel form {name} image {n}: worst row figure {e:.2e}")
        assert e < 1e-9, name


@pytest.mark.parametrize("name", ["a-bands", "b"])
def test_teeth_dropped_carried_run(name):
    """At every register -> element transition of the content map: the run that the first
    lane to change carried in registers is lost."""
    case = M.stride_case(name)
    C = case.content.shape[1]
    trans = M.run_path_census(case.c_segs[0], C, detail=True)["transitions"]
    assert trans
    ratios = []
    for tr in trans:
        drop = M.carried_run_elements(case.c_segs[0], C, *tr)
        assert len(drop) >= 8  # carried over a step boundary: more than one word
        ratios.append(_row_ratio(case, 0, drop))
    print(f"teeth {name}: carried run of one lane dropped, per-row bar missed by "
          f"{min(ratios):.0f}x .. {max(ratios):.0f}x over {len(trans)} transitions")
    assert min(ratios) >= TEETH, (name, ratios)


@pytest.mark.parametrize("name", ["a-bands", "c", "e"])
def test_teeth_dropped_last_step(name):
    """For every slice by itself: its last, partly active step is not walked."""
    case = M.stride_case(name)
    unit, slices = M.plane_slices(case.c_segs[0].size, case.content.shape[1])
    ratios = []
    for lo, hi in slices:
        last = lo + (-(-(hi - lo) // M.SEG_THREADS) - 1) * M.SEG_THREADS
        assert lo < last and 0 < hi - last < M.SEG_THREADS
        ratios.append(_row_ratio(case, 0, np.arange(unit * last, unit * hi)))
    print(f"teeth {name}: last step of one slice ({hi - last} lanes) dropped, per-row bar "
          f"missed by {min(ratios):.0f}x .. {max(ratios):.0f}x over {len(slices)} slices")
    assert min(ratios) >= TEETH, (name, ratios)


@pytest.mark.parametrize("name", ["a-bands", "a-mixed", "c", "d", "e"])
def test_teeth_slice_starts_one_word_late(name):
    """For every slice s >= 1 by itself: its first word (pixel, where HW % 4 != 0) is not
    walked."""
    case = M.stride_case(name)
    unit, slices = M.plane_slices(case.c_segs[0].size, case.content.shape[1])
    ratios = [_row_ratio(case, 0, np.arange(unit * lo, unit * lo + unit)) for lo, _ in slices[1:]]
    print(f"teeth {name}: slice starts one {'word' if unit == 4 else 'pixel'} late, per-row bar "
          f"missed by {min(ratios):.0f}x .. {max(ratios):.0f}x over {len(ratios)} slices")
    assert min(ratios) >= TEETH, (name, ratios)


@pytest.mark.parametrize("name", ["a-bands", "a-speckle", "a-mixed", "c", "e"])
def test_teeth_apply_chunk_base(name):
    """Apply chunk 1 reads the content and the labels at chunk 0's base."""
    case = M.stride_case(name)
    C = case.content.shape[1]
    x = case.content[0].numpy().reshape(C, -1)
    lab = case.c_segs[0].reshape(-1)
    n1 = min(x.shape[1], 2 * M.APPLY_ELEMS) - M.APPLY_ELEMS
    assert n1 > 0
    xs, ls = x.copy(), lab.copy()
    xs[:, M.APPLY_ELEMS:M.APPLY_ELEMS + n1] = x[:, :n1]
    ls[M.APPLY_ELEMS:M.APPLY_ELEMS + n1] = lab[:n1]
    wrong = M.apply_rows(xs, ls, case.rows[0])
    ref = case.out[0].reshape(C, -1)
    sl = slice(M.APPLY_ELEMS, 2 * M.APPLY_ELEMS)
    ratio = rel_l2(wrong[:, sl], ref[:, sl]) / TOL_STATS
    pooled = rel_l2(wrong, ref) / TOL_STATS
    print(f"teeth {name}: apply chunk 1 at chunk 0's base, chunk bar missed by {ratio:.0f}x "
          f"(pooled {pooled:.0f}x)")
    assert ratio >= TEETH and pooled >= TEETH


@pytest.mark.parametrize("name", list(M.STRIDE_SHAPES))
def test_teeth_swapped_style_rows(name):
    """For every valid label by itself: std_s and mean_s change places."""
    case = M.stride_case(name)
    ratios = []
    for lab in np.nonzero(case.counts[0, :, 2])[0]:
        rows = case.rows[0].copy()
        rows[:, lab, 2], rows[:, lab, 3] = case.rows[0][:, lab, 3], case.rows[0][:, lab, 2]
        out = M.apply_rows(case.content[0].numpy(), case.c_segs[0], rows)
        ratios.append(min(rel_l2(out, case.out[0]),
                          max(M.row_errors(rows, case.rows[0], case.counts[0]))) / TOL_STATS)
    print(f"teeth {name}: std_s and mean_s swapped for one label, output and row bars missed "
          f"by {min(ratios):.0f}x .. {max(ratios):.0f}x over {len(ratios)} labels")
    assert min(ratios) >= TEETH, (name, ratios)
