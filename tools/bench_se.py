"""SE channel attention timings (one MI355X).

    python tools/bench_se.py [--reps 20] [--rounds 5] [--out profiles/se_attention/bench.json]
    python tools/bench_se.py --residual-only      # the A/B yardstick alone (tools/ab_se.sh)

Each launch of one SE block (rpst.ops.se_bottleneck) at (N, 32, 512, 512), N = 2 and 16, in
the same process, alternating, after a warm-up: `rounds` timed windows of `reps` calls each
(HIP events on the launch stream), the median window per call reported with the windows'
min / max. GB/s are algorithmic bytes over the median, in passes of 4 N C H W bytes: conv1
reads x and writes h1 (2), conv2 reads h1 and writes h2 (2), the gated conv reads h2 and x and
writes out (3); the block is 7 passes, set against the measured copy bandwidth (6.29 TB/s,
VERDICT.md). The plain 1x1 conv with a residual (rpst_conv2d: act, then + residual) moves the
same bytes as the gated one and is its yardstick.

Then MultiScaleAdaINRPNet.test at 512x512, B = 1 and 8, with bench.py's MULTISCALE_CONFIG at
hidden 32: attention none, se, and se with use_mask (label maps already on the device).

--residual-only times the plain residual conv alone and uses no entry point older libraries
lack, so RPST_LIB can point at the parent commit's library (tools/ab_se.sh)."""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "rp-style-transfer_amd"))

import torch  # noqa: E402

COPY_TBPS = 6.29
C, HW = 32, 512
BATCHES = (2, 16)


def window(fn, reps):
    s = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(s)
    for _ in range(reps):
        fn()
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def medians(fns, reps, rounds):
    """name -> (median, min, max) ms per call over `rounds` windows, candidates alternating."""
    for fn in fns.values():  # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(window(fn, reps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}


def row(op, shape, t, passes=None, **extra):
    r = {"op": op, "shape": list(shape), "ms": round(t[0], 4), "ms_min": round(t[1], 4),
         "ms_max": round(t[2], 4)}
    if passes:
        n, c, h, w = shape
        r["passes"] = passes
        r["GBps"] = round(passes * 4.0 * n * c * h * w / t[0] / 1e6, 1)
    r.update(extra)
    print(json.dumps(r), flush=True)
    return r


def residual_conv(dev, n):
    """The plain-residual 1x1 conv of the gated launch's shape -> (fn, operands)."""
    from rpst import ops
    g = torch.Generator(device=dev).manual_seed(n)
    x = torch.rand((n, C, HW, HW), device=dev, generator=g)
    res = torch.rand((n, C, HW, HW), device=dev, generator=g) - 0.5
    w = (torch.rand((C, C, 1, 1), device=dev, generator=g) - 0.5) * 0.3
    b = torch.rand((C,), device=dev, generator=g) * 0.1
    pk = ops.pack_conv_weight(w)
    out = torch.empty_like(x)
    return (lambda: ops.conv2d(x, pk, b, C, 1, relu=True, residual=res, out=out)), (x, res, pk, b)


def bench_residual(dev, reps, rounds):
    rows = []
    for n in BATCHES:
        fn, _ = residual_conv(dev, n)
        t = medians({"conv1x1_residual": fn}, reps, rounds)["conv1x1_residual"]
        rows.append(row("conv1x1_residual", (n, C, HW, HW), t, 3))
    return rows


def bench_block(dev, reps, rounds):
    import network as net
    from rpst import ops, plan, synth
    rows = []
    for n in BATCHES:
        shape = (n, C, HW, HW)
        blk = net.Conv2dBlock(3, C, 3, 1, padding=1, attention="se")
        synth.synth_module_(torch.nn.ModuleList([blk]), 5)  # keys '0.attention_block. ...'
        se = blk.attention_block.eval().to(dev)
        plain, (x, res, _, _) = residual_conv(dev, n)
        (p1, b1), (p2, b2), (p3, b3), w3 = plan.se_folded(se)
        fa, fb = se.se.fc[0].weight.detach(), se.se.fc[2].weight.detach()
        h1 = ops.conv2d(x, p1, b1, C, 1, relu=True)
        h2, mean_h2, _ = ops.conv2d_stats(h1, p2, b2, C, 3, relu=True)
        gate = ops.se_gate(mean_h2, w3, b3, fa, fb)
        with torch.no_grad():
            fns = {
                "conv1_1x1": lambda: ops.conv2d(x, p1, b1, C, 1, relu=True),
                "conv2_3x3_stats": lambda: ops.conv2d_stats(h1, p2, b2, C, 3, relu=True),
                "se_gate": lambda: ops.se_gate(mean_h2, w3, b3, fa, fb),
                "conv3_gated": lambda: ops.conv2d_gated(h2, p3, b3, gate, x, C, 1),
                "conv3_gated_stats": lambda: ops.conv2d_gated(h2, p3, b3, gate, x, C, 1,
                                                              stats=True),
                "conv1x1_residual": plain,
                "se_block": lambda: ops.se_bottleneck(x, se),
                "se_block_stats": lambda: ops.se_bottleneck(x, se, stats=True),
            }
            t = medians(fns, reps, rounds)
        passes = {"conv1_1x1": 2, "conv2_3x3_stats": 2, "conv3_gated": 3, "conv3_gated_stats": 3,
                  "conv1x1_residual": 3, "se_block": 7, "se_block_stats": 7}
        floor_ms = 7 * 4.0 * n * C * HW * HW / (COPY_TBPS * 1e9)
        for k in fns:
            extra = {}
            if k.startswith("se_block"):
                extra = {"copy_floor_ms": round(floor_ms, 4),
                         "x_copy_floor": round(t[k][0] / floor_ms, 2)}
            if k.startswith("conv3_gated"):
                extra = {"vs_residual": round(t[k][0] / t["conv1x1_residual"][0], 3)}
            rows.append(row(k, shape, t[k], passes.get(k), **extra))
        del x, res, h1, h2
        torch.cuda.empty_cache()
    return rows


def bench_net(dev, reps, rounds):
    import bench
    import network as net
    from rpst import synth
    from tools.bench_masked import label_map
    rows = []
    for b in (1, 8):
        c = torch.from_numpy(synth.image(1, (b, 3, HW, HW))).to(dev)
        s = torch.from_numpy(synth.image(2, (b, 3, HW, HW))).to(dev)
        cseg, sseg = label_map(b, HW, HW, 4, 1).to(dev), label_map(b, HW, HW, 4, 2).to(dev)
        fns = {}
        for name, attention, masked in (("multiscale_test", "none", False),
                                        ("multiscale_test_se", "se", False),
                                        ("multiscale_test_se_masked", "se", True)):
            cfg = dict(bench.MULTISCALE_CONFIG, hidden_dim=C, attention=attention,
                       use_mask=masked)
            m = net.MultiScaleAdaINRPNet(cfg, copy.deepcopy(net.vgg))
            synth.synth_module_(m, 10)
            m = m.to(dev)
            kw = dict(c_mask_path=cseg, s_mask_path=sseg) if masked else {}
            fns[name] = (lambda m=m, kw=kw: m.test(c, s, **kw))
        t = medians(fns, reps, rounds)
        for k in fns:
            rows.append(row(k, (b, 3, HW, HW), t[k]))
        del fns
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--residual-only", action="store_true")
    ap.add_argument("--no-net", action="store_true", help="the SE block's launches only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se_attention", "bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_se: no GPU (timings are taken on the MI355X only)")
    dev = torch.device("cuda:0")
    if a.residual_only:
        # an older library lacks the SE entry points: bind only what it exports
        from rpst import _lib
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in [k for k in _lib.SIGNATURES if not hasattr(lib, k)]:
            del _lib.SIGNATURES[name]
        bench_residual(dev, a.reps, a.rounds)
        return
    rows = bench_block(dev, a.reps, a.rounds) + ([] if a.no_net else bench_net(dev, a.reps, a.rounds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "reps": a.reps, "rounds": a.rounds,
                   "copy_TBps": COPY_TBPS, "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
