"""plan.lower(): which launches a compiled conv plan becomes, pinned on the host. lower()
touches no tensor and no device; its only library calls are the host-only algorithm queries
(test_abi.py::test_conv_algorithm_choice_is_host_only), which pick F(4x4) for any supported
3x3 conv with Cin >= 16 at any size, so 8x8 maps suffice."""
import pytest
import torch
import torch.nn as nn

from rpst import ops, plan

SHAPE = (1, 16, 8, 8)


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in ("RPST_CONV_ALGO", "RPST_CONV_NARROW", "RPST_POOL_EPILOGUE", "RPST_W4Q"):
        monkeypatch.delenv(k, raising=False)


def _pooled_stack():
    return plan.compile_layers([nn.Conv2d(16, 16, 3, padding=1), nn.ReLU(),
                                nn.MaxPool2d(2, 2, ceil_mode=True),
                                nn.Conv2d(16, 32, 3, padding=1), nn.ReLU()])


def _conv3(cin=16, cout=16):
    return [nn.ReflectionPad2d(1), nn.Conv2d(cin, cout, 3), nn.ReLU()]


def _conv7():
    return [nn.ReflectionPad2d(3), nn.Conv2d(16, 16, 7), nn.LeakyReLU(0.2)]


def _ops(launches):
    return [rec.op for rec in launches]


def test_pooled_output_epilogue_by_default():
    steps = _pooled_stack()
    a, b = plan.lower(steps, SHAPE)
    assert (a.op, a.step, a.in_op, a.pooled, a.takes) == ("conv2d_pool", steps[0], ops.IN_NONE,
                                                          True, ())
    # the second conv's pool is already done: it reads the pooled map as a plain input
    assert (b.op, b.step, b.in_op, b.pooled, b.takes) == ("conv2d", steps[1], ops.IN_NONE,
                                                          False, ())


def test_separate_pool_pass_without_the_epilogue(monkeypatch):
    monkeypatch.setenv("RPST_POOL_EPILOGUE", "0")
    steps = _pooled_stack()
    recs = plan.lower(steps, SHAPE)
    assert _ops(recs) == ["conv2d", "maxpool2x2_ceil", "conv2d"]
    assert recs[1].step is None and [r.in_op for r in recs] == [ops.IN_NONE] * 3
    assert not any(r.pooled for r in recs)


def test_direct_algorithm_keeps_the_pool_in_the_loader(monkeypatch):
    monkeypatch.setenv("RPST_CONV_ALGO", "direct")
    recs = plan.lower(_pooled_stack(), SHAPE)
    assert _ops(recs) == ["conv2d", "conv2d"]
    assert [r.in_op for r in recs] == [ops.IN_NONE, ops.IN_MAXPOOL2]


def test_stats_last_takes_the_statistics_epilogue():
    recs = plan.lower(_pooled_stack(), SHAPE, stats_last=True)
    assert _ops(recs) == ["conv2d_pool", "conv2d_stats"]
    assert recs[-1].takes == ("store_n",) and recs[-1].in_op == ops.IN_NONE


def test_pair_read_of_a_plain_first_conv():
    steps = plan.compile_layers(_conv3() + _conv3())
    recs = plan.lower(steps, SHAPE, SHAPE)
    assert _ops(recs) == ["conv2d_pair", "conv2d"]
    assert recs[0].takes == ("x2",) and recs[0].step is steps[0] and recs[1].takes == ()
    # unequal batch sizes pair too (the 3x3 / 1x1 kernel takes any split)
    assert _ops(plan.lower(steps, SHAPE, (3, 16, 8, 8))) == ["conv2d_pair", "conv2d"]


def test_pair_falls_back_to_cat_for_an_adain_first_conv():
    recs = plan.lower(plan.compile_layers(_conv3() + _conv3()), SHAPE, SHAPE,
                      first_in_op=ops.IN_ADAIN)
    assert _ops(recs) == ["cat", "conv2d", "conv2d"]
    assert (recs[1].in_op, recs[1].takes) == (ops.IN_ADAIN, ("aux",))
    assert (recs[2].in_op, recs[2].takes) == (ops.IN_NONE, ())


def test_pair_falls_back_to_cat_for_a_one_conv_plan_with_stats():
    recs = plan.lower(plan.compile_layers(_conv3()), SHAPE, SHAPE, stats_last=True)
    assert _ops(recs) == ["cat", "conv2d_stats"]


def test_7x7_first_conv_reads_two_equal_halves():
    steps = plan.compile_layers(_conv7())
    (rec,) = plan.lower(steps, SHAPE, SHAPE)
    assert (rec.op, rec.step, rec.takes) == ("conv2d_k7", steps[0], ("x2",))


def test_7x7_first_conv_over_unequal_halves_gets_the_concatenation():
    recs = plan.lower(plan.compile_layers(_conv7()), SHAPE, (2, 16, 8, 8))
    assert _ops(recs) == ["cat", "conv2d_k7"] and recs[1].takes == ()


def test_last_7x7_conv_takes_its_statistics_from_the_written_output():
    recs = plan.lower(plan.compile_layers(_conv3() + _conv7()), SHAPE, stats_last=True)
    assert _ops(recs) == ["conv2d", "conv2d_k7", "calc_mean_std"]


def test_trailing_pool_and_upsample_are_stand_alone_launches():
    pool = plan.compile_layers(_conv3() + [nn.MaxPool2d(2, 2, ceil_mode=True)])
    assert _ops(plan.lower(pool, SHAPE)) == ["conv2d", "maxpool2x2_ceil"]
    up = plan.compile_layers(_conv3() + [nn.Upsample(scale_factor=2, mode="nearest")])
    assert _ops(plan.lower(up, SHAPE)) == ["conv2d", "upsample_nearest2x"]
    assert _ops(plan.lower(pool, SHAPE, stats_last=True))[-1] == "calc_mean_std"


def test_skip_adain_first_conv():
    recs = plan.lower(plan.compile_layers(_conv3() + _conv3()), SHAPE,
                      first_in_op=ops.IN_ADD_ADAIN)
    assert _ops(recs) == ["conv2d_skip_adain", "conv2d"]
    assert (recs[0].in_op, recs[0].takes) == (ops.IN_ADD_ADAIN, ("content", "aux"))
    with pytest.raises(NotImplementedError, match="skip-AdaIN conv with statistics"):
        plan.lower(plan.compile_layers(_conv3()), SHAPE, first_in_op=ops.IN_ADD_ADAIN,
                   stats_last=True)


def test_colour_mix_first_conv():
    recs = plan.lower(plan.compile_layers(_conv3() + _conv3()), SHAPE, first_mix=True)
    assert _ops(recs) == ["conv2d_mix", "conv2d"] and recs[0].takes == ("mix",)
    pooled_first = plan.compile_layers([nn.MaxPool2d(2, 2, ceil_mode=True)] + _conv3())
    with pytest.raises(NotImplementedError, match="mixed first conv with an input op"):
        plan.lower(pooled_first, SHAPE, first_mix=True)
    with pytest.raises(NotImplementedError, match="first conv already has an input op"):
        plan.lower(pooled_first, SHAPE, first_in_op=ops.IN_ADAIN)


def test_shapes_propagate_through_pool_and_upsample():
    """An odd map through [conv, pool + conv, upsample + conv]: the queries see ceil-halved
    and doubled sizes; here only the record sequence and operators are pinned."""
    steps = plan.compile_layers(_conv3() + [nn.MaxPool2d(2, 2, ceil_mode=True)] + _conv3()
                                + [nn.Upsample(scale_factor=2, mode="nearest")] + _conv3())
    recs = plan.lower(steps, (2, 16, 7, 9))
    assert _ops(recs) == ["conv2d_pool", "conv2d", "conv2d"]
    assert [r.in_op for r in recs] == [ops.IN_NONE, ops.IN_NONE, ops.IN_UPSAMPLE2]


def test_refusals_come_from_lower(monkeypatch):
    """run() refuses through lower(), before any launch: the refusals of
    test_abi.py::test_plan_rejects_unfused_first_transform and
    test_ld_cpu.py::test_plan_7x7_refuses_loader_operators, on lower() itself and on run()
    with every ops launch made to fail."""
    for name in ("conv2d", "conv2d_k7", "conv2d_mix", "upsample_nearest2x", "calc_mean_std"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("launched before refusing"))
    up = [plan.OpStep(ops.IN_UPSAMPLE2)]
    k7 = plan.compile_layers([nn.ReflectionPad2d(3), nn.Conv2d(8, 8, 7)])
    x4, x8 = torch.zeros(1, 4, 2, 2), torch.zeros(1, 8, 8, 8)
    cases = ((up, x4, dict(first_mix=True), "first_mix"),
             (up, x4, dict(first_in_op=ops.IN_ADAIN), "first_in_op"),
             ([], x4, dict(first_mix=True), "first_mix"),
             (k7, x8, dict(first_in_op=ops.IN_ADAIN), "7x7"),
             (k7, x8, dict(first_mix=True), "7x7"))
    for steps, x, kw, msg in cases:
        with pytest.raises(NotImplementedError, match=msg):
            plan.lower(steps, x.shape, **kw)
        if "first_mix" in kw:
            kw = dict(first_mix=(None, None))
        with pytest.raises(NotImplementedError, match=msg):
            plan.run(steps, x, **kw)
